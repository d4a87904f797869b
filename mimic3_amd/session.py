"""Host-side mirror of the one interface Mimic 3 uses on its hot path.

``Mimic3Voice`` keeps an ``onnxruntime.InferenceSession`` in ``self.onnx_model`` and calls exactly
``self.onnx_model.run(None, inputs)[0].squeeze()`` (``mimic3_tts/voice.py:230``); the session is built in
``Mimic3Voice._load_model`` (``voice.py:378-407``) from ``onnxruntime.SessionOptions()`` with
``graph_optimization_level`` / ``use_deterministic_compute`` assigned and ``providers=None`` or
``["CUDAExecutionProvider"]`` (``tts.py:590-593``).  The classes below keep those names, argument
meanings and error behaviour (Python exceptions, never partial audio) and forward to the MI355X engine
through the C ABI (``include/mi355vits.h``).  There is no CPU execution path here.

Voice files: the reference passes ``<voice_dir>/generator.onnx`` (``voice.py:273``).  The engine reads the
voice from ``generator.m355`` beside it (weights + hyper-parameters, written by ``mimic3_amd.weights.save`` or
``python -m mimic3_amd.onnx_import``) when that exists and belongs to the ``.onnx`` (the ``.onnx`` is absent or an
empty placeholder, or the container's trailer records exactly this file's size and sha256); otherwise the ONNX
initialisers are converted in memory at load time.  A path that already ends in ``.m355`` is used as is.
"""
from __future__ import annotations

import itertools
import os
import threading
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _native
from .config import VitsConfig, tx_class


class GraphOptimizationLevel:
    """Same member names as ``onnxruntime.GraphOptimizationLevel`` (``voice.py:397-399`` sets
    ``ORT_DISABLE_ALL`` on armv7l).  The engine has a fixed launch sequence, so the level is recorded only."""

    ORT_DISABLE_ALL = 0
    ORT_ENABLE_BASIC = 1
    ORT_ENABLE_EXTENDED = 2
    ORT_ENABLE_ALL = 99


class SessionOptions:
    """Attribute bag with the fields the reference assigns (``voice.py:392-401``)."""

    def __init__(self):
        self.graph_optimization_level = GraphOptimizationLevel.ORT_ENABLE_ALL
        self.use_deterministic_compute = False
        self.intra_op_num_threads = 0
        self.inter_op_num_threads = 0
        self.log_severity_level = 2
        # engine extensions (not in onnxruntime)
        self.device_id: Optional[int] = None
        self.seed: Optional[int] = None
        # caller-side micro-batching: concurrent single-utterance run() calls of the server's
        # worker threads that arrive within this window are synthesised as ONE batched engine call (a batch is
        # bitwise equal to separate calls).  0 = off.  Also MI355VITS_MICROBATCH_MS.
        self.micro_batch_window_ms: float = float(os.environ.get("MI355VITS_MICROBATCH_MS", "0") or 0)
        self.micro_batch_max: int = 64
        # engine handles (each with its own HIP stream and workspace) that concurrent run() calls are spread over.
        # The server's worker threads call run() on one shared session without a lock (voice.py:277-292); with one
        # lane those calls queue up behind each other, with two the launch-bound text-encoder / duration-predictor
        # half of one request overlaps the matrix-core half of another (+10 % throughput at batch 32).
        # Results do not depend on the lane.  Also MI355VITS_LANES.
        self.lanes: int = max(1, int(os.environ.get("MI355VITS_LANES", "1") or 1))
        # in-process multi-GPU (SURVEY.md §8f N2 "device round-robin"): the unchanged mimic3-server runs its
        # --num-threads synthesis workers in ONE process on ONE shared session (mimic3_http/__main__.py:53-61,
        # voice.py:277-292), so using the 8 GPUs of a node behind it means this session owns all of them.
        # A list of device indices, or "all"; `lanes` is then per device, the weights are uploaded once per device and
        # shared by its lanes, and every call goes to the least-loaded device.  None = one device (device_id /
        # provider options / MI355VITS_DEVICE / LOCAL_RANK).  Also MI355VITS_DEVICES="0,1,2,3" or "all".
        self.devices: Union[None, str, Sequence[int]] = os.environ.get("MI355VITS_DEVICES") or None
        # matrix-core path of the dense convs on every handle of this session: "bf16x3" (default, f32-grade), "f32",
        # "bf16w" (BASELINE configs[4]: bf16 weights, reduced precision, same utterance lengths), "f16x2".  None = the
        # library's own default (environment MI355VITS_MATH, read when a handle is created).  include/mi355vits.h.
        self.math: Optional[str] = None


class NodeArg:
    def __init__(self, name: str, type_: str, shape: Sequence[Any]):
        self.name = name
        self.type = type_
        self.shape = list(shape)

    def __repr__(self):
        return f"NodeArg(name='{self.name}', type='{self.type}', shape={self.shape})"


class InvalidArgument(ValueError):
    """Bad feed (what onnxruntime reports as ``InvalidArgument``)."""


def resolve_voice_file(path: Union[str, os.PathLike]) -> Union[str, bytes]:
    """What to hand the engine for the model path Mimic 3 passes (``voice.py:273,403``): the ``.m355`` container
    beside it when there is one, otherwise the ONNX file's initialisers converted in memory
    (``mimic3_amd.onnx_import``).  ``python -m mimic3_amd.onnx_import generator.onnx`` writes the
    container once so that later loads skip the conversion."""
    p = os.fspath(path)
    if p.endswith(".m355"):
        if not os.path.isfile(p):
            raise FileNotFoundError(f"{p} not found")
        return p
    cand = os.path.splitext(p)[0] + ".m355"
    if os.path.isfile(cand) and _container_belongs_to(cand, p):
        return cand
    if not os.path.isfile(p):
        raise FileNotFoundError(f"neither {p} nor {cand} found (see INTEGRATION.md)")
    from . import onnx_import
    with open(p, "rb") as f:
        blob = f.read()
    try:
        return onnx_import.onnx_to_m355_bytes(blob, onnx_import.load_voice_config(p), p)
    except onnx_import.OnnxImportError as e:
        raise InvalidArgument(f"cannot load {p}: {e}") from e


def _container_belongs_to(m355_path: str, onnx_path: str) -> bool:
    """Explicit rule (no timestamps): the container stands in for ``onnx_path`` when that file is absent or an empty
    placeholder, or when the container's trailer (``weights.source_record``) names exactly that file — same size and
    same sha256.  A re-downloaded / replaced ``.onnx`` therefore falls back to in-memory conversion."""
    if not os.path.isfile(onnx_path):
        return True
    size = os.path.getsize(onnx_path)
    if size == 0:
        return True
    from . import weights as W

    rec = W.read_source_record(m355_path)
    if rec is None or rec[0] != size:
        return False
    import hashlib

    h = hashlib.sha256()
    with open(onnx_path, "rb") as f:
        for chunk in iter(lambda: f.read(1 << 22), b""):
            h.update(chunk)
    return h.digest() == rec[1]


def _model_bytes(blob: bytes) -> bytes:
    """``InferenceSession(model_bytes)``: an ``.m355`` container as is, anything else is taken for an ONNX model."""
    if blob[:8] == b"M355VITS":
        return blob
    from . import onnx_import
    try:
        return onnx_import.onnx_to_m355_bytes(blob)
    except onnx_import.OnnxImportError as e:
        raise InvalidArgument(f"cannot load model bytes: {e}") from e


def _device_from_providers(providers, provider_options, sess_options) -> int:
    if sess_options is not None and getattr(sess_options, "device_id", None) is not None:
        return int(sess_options.device_id)
    dev = None
    if providers:
        for i, p in enumerate(providers):
            opts = None
            if isinstance(p, (tuple, list)) and len(p) == 2:
                p, opts = p
            elif provider_options and i < len(provider_options):
                opts = provider_options[i]
            if not isinstance(p, str):
                raise InvalidArgument(f"bad provider entry: {p!r}")
            if opts and "device_id" in opts:
                dev = int(opts["device_id"])
    if dev is None:
        dev = int(os.environ.get("MI355VITS_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    return dev


def _resolve_devices(spec, default_device: int, library=None) -> List[int]:
    """``SessionOptions.devices`` -> list of device indices (``None``: the single default device)."""
    if spec is None or spec == "" or spec == []:
        return [int(default_device)]
    lib = library or _native.default_library()
    n = lib.device_count()
    if isinstance(spec, str):
        if spec.strip().lower() == "all":
            if n < 1:
                raise RuntimeError("no HIP device available (the MI355X engine has no CPU fallback)")
            return list(range(n))
        try:
            spec = [int(t) for t in spec.replace(";", ",").split(",") if t.strip() != ""]
        except ValueError:
            raise InvalidArgument(f"bad device list {spec!r} (expected e.g. '0,1,2,3' or 'all')") from None
    devs = [int(d) for d in spec]
    if not devs or len(set(devs)) != len(devs) or any(d < 0 or d >= n for d in devs):
        raise InvalidArgument(f"bad device list {devs!r}: {n} device(s) visible")
    return devs


class _LanePool:
    """Engine handles shared by the caller threads, first come first served.  A released handle is handed straight to
    the longest-waiting caller (no barging): with plain lock / queue semantics a worker that has just finished can
    grab the handle again before the notified waiter wakes up, and some callers starve for seconds under load.
    With several devices a caller gets a free lane on the device that has the fewest calls in flight (ties: the device
    used least recently), so concurrent requests spread over the GPUs before they stack up on one."""

    def __init__(self, engines):
        from collections import deque

        self._free = list(engines)
        self._shut = False
        self._waiters = deque()
        self._lock = threading.Lock()
        self.size = len(engines)
        self._busy: Dict[int, int] = {}
        self._last_use: Dict[int, int] = {}
        self._tick = 0
        for e in engines:
            self._busy.setdefault(e.device, 0)
            self._last_use.setdefault(e.device, -1)
        self.calls_per_device: Dict[int, int] = {d: 0 for d in self._busy}

    def _take(self, eng):
        self._tick += 1
        self._busy[eng.device] += 1
        self._last_use[eng.device] = self._tick
        self.calls_per_device[eng.device] += 1
        return eng

    def acquire(self):
        with self._lock:
            if self._shut:
                raise RuntimeError("session is closed")
            if self._free and not self._waiters:
                best = min(range(len(self._free)), key=lambda i: (self._busy[self._free[i].device],
                                                                    self._last_use[self._free[i].device], i))
                return self._take(self._free.pop(best))
            slot = [None]
            ev = threading.Event()
            self._waiters.append((ev, slot))
        try:
            ev.wait()
        except BaseException:
            # interrupted while queued: leave the queue, or give back the lane that was handed over meanwhile
            with self._lock:
                if slot[0] is None:
                    try:
                        self._waiters.remove((ev, slot))
                    except ValueError:
                        pass
                    raise
            self.release(slot[0])
            raise
        if slot[0] is None:  # woken by shutdown(): the session was closed while this caller queued
            raise RuntimeError("session is closed")
        return slot[0]

    def shutdown(self) -> None:
        """After close() has collected every lane: later callers fail at once, callers still queued are woken with an error
        (they would wait forever: no lane is ever released again)."""
        with self._lock:
            self._shut = True
            waiters, self._waiters = list(self._waiters), type(self._waiters)()
        for ev, _slot in waiters:
            ev.set()

    def release(self, eng) -> None:
        with self._lock:
            self._busy[eng.device] -= 1
            if self._waiters:
                ev, slot = self._waiters.popleft()
                slot[0] = self._take(eng)
                ev.set()
            else:
                self._free.append(eng)

    def idle(self) -> int:
        with self._lock:
            return len(self._free)


# run keywords that may differ between the rows of one engine call (mi355vits_run_rows)
_ROW_SETTINGS = ("pcm_volume", "utterance_keys")


class _MicroBatcher:
    """Coalesces concurrent B = 1 requests into batched engine calls (one dispatcher thread per session).

    The reference issues one ``run`` per sentence from each of its ``--num-threads`` synthesis workers
    (``mimic3_http/synthesis.py:88-136``); behind an unchanged API this is where batch parallelism comes from."""

    def __init__(self, session: "InferenceSession", window_s: float, max_batch: int):
        import queue
        import weakref

        # weak: the dispatcher thread must not keep a session (and its engines' HBM) alive after its last user is gone
        self._session_ref = weakref.ref(session)
        self._window = window_s
        self._max = max(1, int(max_batch))
        self._cap = session.config.attention_cap  # the voice's last length-class boundary (config.tx_class)
        self._q: "queue.Queue" = queue.Queue()
        self.batches = 0
        self.requests = 0
        self._count_lock = threading.Lock()
        # batches handed to a lane and not back yet (the dispatcher holds a new batch back while every lane has one)
        self._inflight = 0
        self._inflight_cv = threading.Condition()
        # with several lanes the dispatcher hands each batch to a worker and goes back to collecting, so that one batch
        # can run its launch-bound front half while the previous one is still in its matrix-core back half
        lanes = len(getattr(session, "_engines", [None]))
        self._lanes = max(1, lanes)
        self._pool = None
        if lanes > 1:
            from concurrent.futures import ThreadPoolExecutor

            self._pool = ThreadPoolExecutor(max_workers=lanes, thread_name_prefix="mi355vits-lane")
        self._thread = threading.Thread(target=self._loop, name="mi355vits-microbatch", daemon=True)
        self._thread.start()

    def submit(self, ids, lengths, scales, sid, kw):
        from concurrent.futures import Future

        fut: "Future" = Future()
        self._q.put((ids, lengths, scales, sid, kw, fut))
        return fut

    def _loop(self):
        import queue
        import time

        lanes = self._lanes
        while True:
            first = self._q.get()
            if first is None:
                return
            items = [first]
            stop = False

            def take(timeout):  # one more request into `items`; False when there is none (yet) or the batcher is closing
                nonlocal stop
                try:
                    nxt = self._q.get(timeout=timeout) if timeout > 0 else self._q.get_nowait()
                except queue.Empty:
                    return False
                if nxt is None:
                    self._q.put(None)
                    stop = True
                    return False
                items.append(nxt)
                return True

            # (1) the arrival window — skipped for a lone request on an idle session: nothing is in flight and nothing else has
            # arrived, so waiting could only add latency to the very call the reference makes most (one sentence, voice.py:230);
            # a burst then forms behind that first call.  (2) while EVERY lane has a batch, keep collecting instead of queueing
            # small batches behind the lanes: under load a batch is everything that arrived while the chip was busy (round 5's
            # fixed window cut 64 closed-loop clients into batches of 8: profiles/r05_serve_bench.log).
            with self._inflight_cv:
                idle = self._inflight == 0
            while len(items) < self._max and not stop and take(0):  # a backlog (the chip was busy) is a batch already
                pass
            if len(items) == 1 and not idle:
                deadline = time.perf_counter() + self._window
                while len(items) < self._max and not stop:
                    left = deadline - time.perf_counter()
                    if left <= 0 or not take(left):
                        break
            while not stop:
                with self._inflight_cv:
                    if self._inflight < lanes:
                        break
                    if len(items) >= self._max:
                        self._inflight_cv.wait(timeout=0.05)  # a full batch waits for a lane, nothing more to collect
                        continue
                if not take(0.0002):
                    with self._inflight_cv:
                        if self._inflight >= lanes:
                            self._inflight_cv.wait(timeout=0.0002)
            while len(items) < self._max and not stop and take(0):  # whatever arrived meanwhile rides along
                pass
            # scales, PCM volume and noise key are per row (mi355vits_run_rows), so requests with any settings share a call; only
            # the output kind and sid presence must agree, and the phoneme-length class: the text encoder picks its attention /
            # FFN kernels by the padded length (<= 128, 256, 512, the voice's attention cap, beyond: config.tx_class), so within
            # a class a row gets the kernels — and the bits — it would get alone
            # A stream request (run_stream) brings one or more rows and what ITS stream of the call looks like ("_stream": order,
            # silences, header, encoding, trim, loudness — per stream, so nothing to group by); its class is that of its padded width,
            # which is what its own call would run at.
            groups: Dict[Any, list] = {}
            for it in items:
                stream = "_stream" in it[4]
                bucket = tx_class(int(it[0].shape[1]) if stream else int(it[1][0]), self._cap)
                kind = tuple(sorted((k, v) for k, v in it[4].items() if k not in _ROW_SETTINGS and k != "_stream"))
                key = (it[3] is None, kind, bucket)
                groups.setdefault(key, []).append(it)
            batches = []
            for group in groups.values():
                if "_stream" not in group[0][4]:
                    batches.append(group)
                    continue
                part, rows = [], 0  # stream requests: no engine call above micro_batch_max rows
                for it in group:
                    if part and rows + it[0].shape[0] > self._max:
                        batches.append(part)
                        part, rows = [], 0
                    part.append(it)
                    rows += it[0].shape[0]
                batches.append(part)
            for group in batches:
                with self._inflight_cv:
                    self._inflight += 1
                if self._pool is not None:
                    self._pool.submit(self._run_counted, group)
                else:
                    self._run_counted(group)

    def _run_counted(self, group):
        released = [False]

        def lane_done():  # the batch's lane is free again: the dispatcher may hand out the next batch
            if not released[0]:
                released[0] = True
                with self._inflight_cv:
                    self._inflight -= 1
                    self._inflight_cv.notify_all()

        try:
            self._run_group(group, lane_done)
        finally:
            lane_done()

    def _run_stream_group(self, group):
        """Stream requests as ONE ``run_streams`` call: every request's rows side by side, one stream of the block per request, and
        each caller's result a view of that shared block (no slice is copied)."""
        try:
            tx = max(int(g[0].shape[1]) for g in group)
            B = sum(int(g[0].shape[0]) for g in group)
            ids = np.zeros((B, tx), np.int64)
            lens = np.zeros(B, np.int64)
            scales = np.zeros((B, 3), np.float32)
            vols, keys, sids, streams = [], [], [], []
            r0 = 0
            for g in group:
                R = int(g[0].shape[0])
                # (run_stream has checked order and lead_samples against the request's OWN rows: adding r0 must never reach a neighbour's)
                _check_stream_rows(g[4]["_stream"].get("order"), g[4]["_stream"].get("lead_samples"), R)
                ids[r0:r0 + R, : g[0].shape[1]] = g[0]
                lens[r0:r0 + R] = g[1]
                scales[r0:r0 + R] = np.asarray(g[2], np.float32).reshape(-1, 3)  # [3] or [R, 3]
                vols += [float(v) for v in np.broadcast_to(np.asarray(g[4].get("pcm_volume", 1.0), np.float64).reshape(-1), (R,))]
                k = g[4].get("utterance_keys")
                keys += [None] * R if k is None else list(k)
                if g[3] is not None:
                    sids += [int(v) for v in np.asarray(g[3]).reshape(-1)]
                st = dict(g[4]["_stream"])
                n = R if st.get("lead_samples") is None else len(np.asarray(st["lead_samples"]).reshape(-1))  # without an order: entries 0 .. n - 1
                st["order"] = (np.arange(n) if st.get("order") is None else np.asarray(st["order"]).reshape(-1)) + r0
                streams.append(st)
                r0 += R
            kw = {k: v for k, v in group[0][4].items() if k not in _ROW_SETTINGS and k not in ("_stream", "_kind")}
            if any(v != 1.0 for v in vols):
                kw["pcm_volume"] = np.asarray(vols, np.float64)
            if any(k is not None for k in keys):
                kw["utterance_keys"] = keys  # rows without a key of their own get base + b (_engine_run)
            session = self._session_ref()
            if session is None:
                raise RuntimeError("session closed")
            out = session._engine_run(ids, lens, scales if (scales != scales[0]).any() else scales[0].copy(),
                                      np.asarray(sids, np.int64) if group[0][3] is not None else None, _streams=streams, **kw)
            del session
            with self._count_lock:
                self.batches += 1
                self.requests += len(group)
            for g, pa in zip(group, out):
                g[5].set_result(pa)
        except BaseException as e:
            if len(group) > 1:
                # a bad request must not poison its batch-mates: fall back to one call per request
                for g in group:
                    if not g[5].done():
                        self._run_stream_group([g])
                return
            for g in group:
                if not g[5].done():
                    g[5].set_exception(e)

    def _run_group(self, group, lane_done=None):
        if "_stream" in group[0][4]:
            return self._run_stream_group(group)
        try:
            tx = max(int(g[0].shape[1]) for g in group)
            B = len(group)
            ids = np.zeros((B, tx), np.int64)
            lens = np.zeros(B, np.int64)
            for b, g in enumerate(group):
                n = int(g[1][0])
                ids[b, :n] = g[0][0, :n]
                lens[b] = n
            sid = None if group[0][3] is None else np.array([int(g[3][0]) for g in group], np.int64)
            kw = {k: v for k, v in group[0][4].items() if k not in _ROW_SETTINGS}
            scales = group[0][2]
            if B > 1:
                # per-row arrays only where the rows differ: a uniform batch takes the plain call, as before
                rows = np.stack([np.asarray(g[2], np.float32).reshape(3) for g in group])
                if (rows != rows[0]).any():
                    scales = rows
                vols = [float(np.asarray(g[4].get("pcm_volume", 1.0), np.float64).reshape(-1)[0]) for g in group]
                if any(v != vols[0] for v in vols):
                    kw["pcm_volume"] = np.asarray(vols, np.float64)
                elif "pcm_volume" in group[0][4]:
                    kw["pcm_volume"] = vols[0]
                keys = [g[4]["utterance_keys"][0] if g[4].get("utterance_keys") is not None else None for g in group]
                if any(k is not None for k in keys):
                    kw["utterance_keys"] = keys  # rows without a key of their own get base + b (_engine_run)
            else:
                kw = dict(group[0][4])
            session = self._session_ref()
            if session is None:
                raise RuntimeError("session closed")
            out = session._engine_run(ids, lens, scales, sid, **kw)
            del session  # (the batch stays "in flight" through the slicing below: handing the next batch out earlier was measured —
            # 19.1k -> 16.9k x real time at 64 clients, the batches shrink from 15.5 to 12.2: profiles/r06_serve_policies.txt)
            with self._count_lock:
                self.batches += 1
                self.requests += B
            for b, g in enumerate(group):
                L = int(out["lengths"][b])
                res = {"lengths": out["lengths"][b:b + 1].copy(), "peaks": out["peaks"][b:b + 1].copy()}
                if "audio" in out:
                    res["audio"] = out["audio"][b:b + 1, :L].copy()
                if "pcm" in out:
                    res["pcm"] = out["pcm"][b:b + 1, :L].copy()
                g[5].set_result(res)
        except BaseException as e:
            if len(group) > 1:
                # a bad request must not poison its batch-mates: fall back to one call per request
                for g in group:
                    if not g[5].done():
                        self._run_group([g], None)
                return
            for g in group:  # every waiter gets its error; nobody hangs
                if not g[5].done():
                    g[5].set_exception(e)

    def close(self):
        import queue

        self._q.put(None)
        on_dispatcher = self._thread is threading.current_thread()
        if not on_dispatcher:
            self._thread.join(timeout=5.0)
        if self._pool is not None:
            self._pool.shutdown(wait=not on_dispatcher)  # batches already handed to a lane finish first
        # requests still queued get an error instead of hanging
        while True:
            try:
                it = self._q.get_nowait()
            except queue.Empty:
                break
            if it is not None and not it[5].done():
                it[5].set_exception(RuntimeError("session closed"))
        if not on_dispatcher and self._thread.is_alive():
            self._q.put(None)  # the drain above may have swallowed the sentinel of a dispatcher that was still busy
            self._thread.join(timeout=5.0)


def _check_stream_rows(order, lead_samples, rows: int) -> None:
    """A stream request's ``order`` / ``lead_samples`` against ITS OWN ``rows`` rows, by the rules the library applies to a call of
    those rows alone — in a shared call the library sees the whole batch, where an index past the request's rows is another
    client's sentence.  Raises ``InvalidArgument`` naming the entry."""
    n = rows
    if order is not None:
        o = np.asarray(order).reshape(-1)
        if o.size and not np.issubdtype(o.dtype, np.integer):
            raise InvalidArgument("'order' must hold integers")
        n = int(o.size)
        if n < 1 or n > rows:
            raise InvalidArgument(f"pack: n = {n} out of range (1 .. batch = {rows})")
        seen: Dict[int, int] = {}
        for i, r in enumerate(int(v) for v in o):
            if r < 0 or r >= rows:
                raise InvalidArgument(f"pack entry {i}: row {r} out of range (batch = {rows})")
            if r in seen:
                raise InvalidArgument(f"pack entry {i}: row {r} appears twice (also entry {seen[r]})")
            seen[r] = i
    if lead_samples is not None:
        lead = np.asarray(lead_samples).reshape(-1)
        if lead.size and not np.issubdtype(lead.dtype, np.integer):
            raise InvalidArgument("'lead_samples' must hold integers")
        if order is None:  # entries 0 .. n - 1, n the number of silences given (as run_packed)
            if lead.size < 1 or lead.size > rows:
                raise InvalidArgument(f"pack: n = {int(lead.size)} out of range (1 .. batch = {rows})")
        elif int(lead.size) != n:
            raise InvalidArgument("'order' and 'lead_samples' must have the same length")


def _encoding_name(encoding) -> str:
    """A packed stream's sample encoding as its lower-case name; ``ValueError`` for anything else."""
    if not isinstance(encoding, str) or encoding.lower() not in _native.ENCODINGS:
        raise ValueError(f"unknown output encoding {encoding!r} (one of {', '.join(_native.ENCODINGS)})")
    return encoding.lower()


_SESSION = object()  # compression=: "whatever the session's output_compression is"


def _compression_name(compression) -> Optional[str]:
    """A packed stream's compression as ``"flac"`` or ``None`` (also for ``"none"``); ``ValueError`` for anything else."""
    if compression is None:
        return None
    if not isinstance(compression, str) or compression.lower() not in ("flac", "none"):
        raise ValueError(f"unknown output compression {compression!r} ('flac' or None)")
    return "flac" if compression.lower() == "flac" else None


def _trim_ratio(db) -> float:
    """An edge-trim threshold in dB below a row's peak as the engine's ratio: ``float(np.float32(10 ** (db / 20)))``; ``None`` =
    off (0.0).  ``db`` must be finite and <= 0, else ``ValueError``."""
    if db is None:
        return 0.0
    db = float(db)
    if not np.isfinite(db) or db > 0.0:
        raise ValueError(f"edge trim threshold must be finite and <= 0 dB, not {db!r}")
    return float(np.float32(10.0 ** (db / 20.0)))


def _loudness_setting(lufs, ceiling_db):
    """A loudness target as the engine's ``(target_lufs, ceiling_dbfs)``; ``None`` = off ``(0.0, ceiling)``.  On: -70 <= lufs < 0 and
    a finite ceiling <= 0 dBFS, else ``ValueError``."""
    ceiling = -1.0 if ceiling_db is None else float(ceiling_db)
    if lufs is None:
        return 0.0, ceiling
    lufs = float(lufs)
    if not (-70.0 <= lufs < 0.0):
        raise ValueError(f"loudness target must be in [-70, 0) LUFS, not {lufs!r}")
    if not np.isfinite(ceiling) or ceiling > 0.0:
        raise ValueError(f"loudness ceiling must be finite and <= 0 dBFS, not {ceiling!r}")
    return lufs, ceiling


def _alignment_levels(alignment) -> bool:
    """``alignment=True`` -> timing only, ``"levels"`` -> peak and rms too; anything else raises ``ValueError``."""
    if alignment is True:
        return False
    if isinstance(alignment, str) and alignment.lower() == "levels":
        return True
    raise ValueError(f"alignment must be False, True or 'levels', not {alignment!r}")


class InferenceSession:
    """Drop-in for the object stored in ``Mimic3Voice.onnx_model``."""

    _seed_counter = itertools.count(0x5EED)

    def __init__(self, path_or_bytes, sess_options: Optional[SessionOptions] = None, providers=None,
                 provider_options=None, **kwargs):
        self._sess_options = sess_options or SessionOptions()
        self._providers = ["MI355XExecutionProvider"]
        device = _device_from_providers(providers, provider_options, self._sess_options)
        library = kwargs.pop("_library", None)  # tests only: an explicit NativeLibrary
        # the rate of every result (Engine.set_output_rate): None = the voice's own; a call's ``sample_rate=`` goes before it
        rate = kwargs.pop("output_sample_rate", None)
        self.output_sample_rate: Optional[int] = int(rate) if rate else None
        # the sample encoding of the packed streams (Engine.set_output_encoding); a call's ``encoding=`` goes before it
        self.output_encoding: str = _encoding_name(kwargs.pop("output_encoding", None) or "s16le")
        # the compression of the packed stream (Engine.set_output_compression): "flac" or None; a call's ``compression=`` goes before it
        self.output_compression: Optional[str] = _compression_name(kwargs.pop("output_compression", None))
        # edge trimming of the packed streams (Engine.set_edge_trim): dB below each row's peak, None = off, and the milliseconds
        # kept around the loud part; a call's ``trim_db=`` / ``trim_keep_ms=`` go before them
        self.edge_trim_db: Optional[float] = kwargs.pop("edge_trim_db", None)
        _trim_ratio(self.edge_trim_db)
        self.edge_trim_keep_ms: float = float(kwargs.pop("edge_trim_keep_ms", 0) or 0)
        if self.edge_trim_keep_ms < 0:
            raise ValueError("edge_trim_keep_ms must be >= 0")
        # loudness target of the packed streams (Engine.set_loudness_target): LUFS, None = off, and the ceiling in dBFS that bounds
        # the gain; a call's ``loudness=`` / ``ceiling_db=`` go before them
        self.loudness_lufs: Optional[float] = kwargs.pop("loudness_lufs", None)
        self.loudness_ceiling_db: float = float(kwargs.pop("loudness_ceiling_db", -1.0))
        _loudness_setting(self.loudness_lufs, self.loudness_ceiling_db)
        # look-ahead peak limiter of the packed streams with a target (Engine.set_loudness_limiter): its window in milliseconds,
        # None = off; a call's ``limiter_ms=`` goes before it.  Milliseconds become samples at the run's rate when a call is made.
        self.loudness_limiter_ms: Optional[float] = kwargs.pop("loudness_limiter_ms", None)
        if self.loudness_limiter_ms is not None:
            ms = float(self.loudness_limiter_ms)
            if not (np.isfinite(ms) and ms > 0.0):
                raise ValueError(f"loudness_limiter_ms must be finite and > 0 (or None = off), not {self.loudness_limiter_ms!r}")
        # what the ceiling bounds (Engine.set_loudness_ceiling_mode): False = the sample peak, True = the 4x oversampled peak; a
        # call's ``true_peak=`` goes before it
        self.loudness_true_peak: bool = bool(kwargs.pop("loudness_true_peak", False))
        if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
            weights = _model_bytes(bytes(path_or_bytes))
            self._model_path = None
        else:
            weights = resolve_voice_file(path_or_bytes)
            self._model_path = weights if isinstance(weights, str) else os.fspath(path_or_bytes)
        lanes = max(1, int(getattr(self._sess_options, "lanes", 1) or 1))
        devices = _resolve_devices(getattr(self._sess_options, "devices", None), device, library)
        # one weight upload per device; further lanes of a device share it (mi355vits_clone).  Lane-major order:
        # consecutive handles sit on different devices.
        firsts = []
        self._engines = []
        try:
            for d in devices:
                firsts.append(_native.Engine(weights, device=d, library=library))
                self._engines.append(firsts[-1])
            for _ in range(lanes - 1):
                for f in firsts:
                    self._engines.append(f.clone())
            if getattr(self._sess_options, "math", None):
                for e in self._engines:
                    e.set_math(self._sess_options.math)
            if self.output_sample_rate:
                try:
                    for e in self._engines:  # a rate the engine refuses fails here, not in the first call
                        e.set_output_rate(self.output_sample_rate)
                except _native.NativeError as e:
                    raise InvalidArgument(str(e)) from None
        except BaseException:
            for e in reversed(self._engines):  # clones before the handles whose weights they share
                e.close()
            self._engines = []
            raise
        self.devices = list(devices)
        self._closed = False
        self._engine = self._engines[0]
        self._free_lanes = _LanePool(self._engines)
        self.config: VitsConfig = self._engine.config
        seed = self._sess_options.seed
        self._seed = int(seed) if seed is not None else next(InferenceSession._seed_counter)
        self._utterances = 0
        self._lock = threading.Lock()
        self.last_lengths: Optional[np.ndarray] = None
        self.last_timing_factor: Optional[np.ndarray] = None  # of the last timed run_pcm16 (the factor every row was fitted with)
        self._batcher: Optional[_MicroBatcher] = None
        if self._sess_options.micro_batch_window_ms and self._sess_options.micro_batch_window_ms > 0:
            self._batcher = _MicroBatcher(self, self._sess_options.micro_batch_window_ms * 1e-3,
                                          self._sess_options.micro_batch_max)

    # ---- onnxruntime surface ----------------------------------------------------------------
    def get_providers(self) -> List[str]:
        return list(self._providers)

    def get_inputs(self) -> List[NodeArg]:
        args = [
            NodeArg("input", "tensor(int64)", ["batch_size", "phonemes"]),
            NodeArg("input_lengths", "tensor(int64)", ["batch_size"]),
            NodeArg("scales", "tensor(float)", [3]),
        ]
        if self.config.is_multispeaker:
            args.append(NodeArg("sid", "tensor(int64)", ["batch_size"]))
        return args

    def get_outputs(self) -> List[NodeArg]:
        return [NodeArg("output", "tensor(float)", ["batch_size", 1, "time"])]

    def run(self, output_names, input_feed: Dict[str, np.ndarray], run_options=None) -> List[np.ndarray]:
        """``run(None, {"input", "input_lengths", "scales"[, "sid"]}) -> [float32 [B, 1, L]]``.

        Rows shorter than the longest one are padding beyond ``last_lengths[b]`` samples (the reference
        only ever calls this with B = 1 and squeezes the result)."""
        if output_names is not None and list(output_names) not in ([], ["output"]):
            raise InvalidArgument(f"unknown output names {output_names!r}; the graph has one output 'output'")
        audio, lengths = self._run(input_feed, want_float=True)["audio"], self.last_lengths
        return [audio[:, None, :]]

    # ---- engine extensions --------------------------------------------------------------------
    def run_pcm16(self, input_feed: Dict[str, np.ndarray], volume=None, direct: bool = False, utterance_keys=None,
                  sample_rate: Optional[int] = None, alignment=False, stretch=None, min_frames=None, target_frames=None,
                  duration_ms=None, speakers=None, gain_db=None, ramp_ms=None, pitch=None, pitch_semitones=None):
        """``run`` + ``audio_float_to_int16`` (``utils.py:237-244``) fused on the GPU, per utterance over its
        valid samples.  Returns ([int16 [L_b]] per row, lengths).

        ``volume`` (percent, like ``Mimic3Settings.volume``): additionally applies
        ``audioop.mul(audio_bytes, 2, volume / 100)`` (``tts.py:542-543``) in the same kernel — same bytes as the host
        call, one pass fewer over the audio.  A sequence gives each row its own volume.  ``direct``: a
        single-utterance call goes straight to a lane instead of through the micro-batcher's queue (a planned request's first
        sentence: two thread hand-overs fewer; same bits).  ``utterance_keys`` ([B] ints): the Philox utterance index of each
        row instead of the session's running count (``reserve_utterances``) — a row's noise, hence its audio at nonzero
        noise scales, then depends on its own inputs only, not on the batch or the moment it rides in.  ``sample_rate``: the
        rate of this call's audio instead of the session's ``output_sample_rate`` (resampled as f32 on the GPU before the int16
        conversion; not a per-row setting: micro-batched requests of different rates never share an engine call).
        ``alignment`` (``True``, or ``"levels"`` for peak and rms too): also where each phoneme sits in its row
        (``mi355vits_fetch_alignment``) — the call then goes straight to a lane, never through the micro-batcher, fetches the
        alignment on that lane before releasing it, and returns (rows, lengths, ``_native.Alignment``).
        Timing in the same run (``mi355vits_run_timed``): ``stretch`` [B, Tx] multiplies each phoneme's duration, ``min_frames``
        [B, Tx] holds a phoneme (a pause symbol) at least that many latent frames, ``target_frames`` [B] fits the row to exactly
        that many latent frames (0 = as predicted), or ``duration_ms`` [B] (0 / ``None`` = as predicted) the same in time:
        ``max(1, round(ms / 1000 * sample_rate / hop))`` frames at the voice's native rate.  Such a call goes straight to a lane,
        never through the micro-batcher; the factors it was fitted with are left in ``last_timing_factor``.
        ``speakers`` (``mi355vits_run_speakers``; a multi-speaker voice): who speaks each row, in place of the feed's ``sid`` (which
        may then be left out) — one entry per row: an ``int`` (that speaker), a dict ``{sid: weight}`` (a blend such as
        ``{12: 0.7, 40: 0.3}``, extrapolation such as ``{12: 1.5, 40: -0.5}`` included) or a 1-D float array of ``gin_channels``
        values (a vector of the caller's own: see ``speaker_embedding``).  Ints and dicts may be mixed in one call; vectors go in a
        call of their own (``ValueError`` otherwise).  Such a call goes straight to a lane, never through the micro-batcher.
        Levels in the same run (``mi355vits_run_levels``): ``gain_db`` — one list per row or a [B, Tx] array — is the gain of each
        phoneme in dB (``-inf`` mutes; converted as ``np.float32(10 ** (dB / 20))``; a list shorter than Tx leaves the rest at 0 dB),
        ``ramp_ms`` (a number or [B]) the half-width of the linear ramp across every phoneme boundary,
        ``round(ms / 1000 * sample_rate)`` samples at the voice's native rate (default 0: steps).  The envelope is applied to the
        waveform on the GPU in front of the int16 conversion.  Such a call goes straight to a lane, never through the micro-batcher.
        Pitch in the same run (``mi355vits_run_pitch``): ``pitch`` — one list per row or a [B, Tx] array — is the pitch multiplier of
        each phoneme (0.5 .. 2; a list shorter than Tx leaves the rest at 1), or ``pitch_semitones`` the same in semitones
        (``np.float32(2 ** (st / 12))``); the two exclude each other.  Each phoneme keeps its duration; this is resampling,
        so formants move with the pitch.  Such a call goes straight to a
        lane, never through the micro-batcher."""
        kw = self._pcm_kw(volume, utterance_keys)
        if sample_rate is not None:
            kw["sample_rate"] = int(sample_rate)
        timing = self._timing_kw(input_feed, stretch, min_frames, target_frames, duration_ms)
        kw.update(timing)
        if speakers is not None:
            kw["speakers"] = speakers
        levels = self._levels_kw(input_feed, gain_db, ramp_ms)
        levels.update(self._pitch_kw(input_feed, pitch, pitch_semitones))
        kw.update(levels)
        if alignment or timing or speakers is not None or levels:
            ids, lengths, sid = self._feed(input_feed, speakers is not None)
            keys = kw.pop("utterance_keys", None)
            out = self._engine_run(ids, lengths, input_feed["scales"], sid, utterance_keys=keys,
                                   _alignment=_alignment_levels(alignment) if alignment else None, want_float=False, want_pcm16=True, **kw)
            out, al = out if alignment else (out, None)
            self.last_lengths = out["lengths"]
            if timing:
                self.last_timing_factor = out["timing_factor"]
            rows = [out["pcm"][b, : int(out["lengths"][b])] for b in range(out["pcm"].shape[0])]
            return (rows, out["lengths"], al) if alignment else (rows, out["lengths"])
        out = self._run(input_feed, _direct=direct, want_float=False, want_pcm16=True, **kw)
        return [out["pcm"][b, : int(out["lengths"][b])] for b in range(out["pcm"].shape[0])], out["lengths"]

    def _timing_kw(self, input_feed, stretch, min_frames, target_frames, duration_ms) -> Dict[str, np.ndarray]:
        """The timing keywords of ``Engine.run`` / ``run_packed`` (empty without any): ``duration_ms`` [B] becomes
        ``target_frames`` at the voice's native rate, ``max(1, round(ms / 1000 * sample_rate / hop))``; 0 / None = no target."""
        kw = {}
        if stretch is not None:
            kw["stretch"] = stretch
        if min_frames is not None:
            kw["min_frames"] = min_frames
        if duration_ms is not None:
            if target_frames is not None:
                raise ValueError("give target_frames or duration_ms, not both")
            B = np.asarray(input_feed["input"]).shape[0]
            ms = np.array([0.0 if m is None else float(m) for m in np.asarray(duration_ms, object).reshape(-1)], np.float64)
            if ms.shape != (B,):
                raise ValueError("duration_ms must have shape [batch]")
            if not np.all(np.isfinite(ms)) or np.any(ms < 0):
                raise ValueError("duration_ms must be finite and >= 0")
            per_ms = self.config.sample_rate / 1000.0 / self.config.hop_length
            target_frames = [0 if m == 0 else max(1, int(round(m * per_ms))) for m in ms]
        if target_frames is not None:
            kw["target_frames"] = target_frames
        return kw

    def _levels_kw(self, input_feed, gain_db, ramp_ms) -> Dict[str, np.ndarray]:
        """The level keywords of ``Engine.run`` / ``run_packed`` (empty without ``gain_db``): ``gain`` [B, Tx] =
        ``np.float32(10 ** (dB / 20))`` (``-inf`` dB = 0), ``ramp_samples`` [B] = ``round(ms / 1000 * sample_rate)`` at the voice's
        native rate."""
        if gain_db is None:
            if ramp_ms is not None:
                raise ValueError("ramp_ms needs gain_db")
            return {}
        shape = np.asarray(input_feed["input"]).shape
        if len(shape) != 2:
            raise ValueError("'input' must have shape [batch, phonemes]")
        B, Tx = shape
        db = np.zeros((B, Tx), np.float64)
        rows = list(gain_db)
        if len(rows) != B:
            raise ValueError("gain_db must have one entry per row")
        for b, r in enumerate(rows):
            r = np.asarray(r, np.float64).reshape(-1)
            if r.size > Tx:
                raise ValueError("gain_db: a row has more entries than the feed has phonemes")
            db[b, : r.size] = r
        if np.any(np.isnan(db)) or np.any(db == np.inf):
            raise ValueError("gain_db must be a number or -inf")
        kw = {"gain": np.float32(10.0 ** (db / 20.0))}
        if ramp_ms is not None:
            ms = np.asarray(ramp_ms, np.float64)
            ms = np.full(B, float(ms)) if ms.ndim == 0 else ms
            if ms.shape != (B,):
                raise ValueError("ramp_ms must be a number or have shape [batch]")
            if not np.all(np.isfinite(ms)) or np.any(ms < 0):
                raise ValueError("ramp_ms must be finite and >= 0")
            kw["ramp_samples"] = np.array([int(round(m / 1000.0 * self.config.sample_rate)) for m in ms], np.int64)
        return kw

    @staticmethod
    def _pitch_kw(input_feed, pitch, pitch_semitones) -> Dict[str, np.ndarray]:
        """The pitch keyword of ``Engine.run`` / ``run_packed`` (empty without either): ``pitch`` [B, Tx], the ratios themselves or
        ``np.float32(2 ** (st / 12))``; rows shorter than Tx are filled with 1."""
        if pitch is None and pitch_semitones is None:
            return {}
        if pitch is not None and pitch_semitones is not None:
            raise ValueError("pitch and pitch_semitones exclude each other")
        shape = np.asarray(input_feed["input"]).shape
        if len(shape) != 2:
            raise ValueError("'input' must have shape [batch, phonemes]")
        B, Tx = shape
        semis = pitch is None
        name = "pitch_semitones" if semis else "pitch"
        v = np.full((B, Tx), 0.0 if semis else 1.0, np.float64)
        rows = list(pitch_semitones if semis else pitch)
        if len(rows) != B:
            raise ValueError(name + " must have one entry per row")
        for b, r in enumerate(rows):
            r = np.asarray(r, np.float64).reshape(-1)
            if r.size > Tx:
                raise ValueError(name + ": a row has more entries than the feed has phonemes")
            v[b, : r.size] = r
        if not np.all(np.isfinite(v)):
            raise ValueError(name + " must be finite")
        return {"pitch": np.float32(2.0 ** (v / 12.0)) if semis else v.astype(np.float32)}

    def run_packed(self, input_feed: Dict[str, np.ndarray], order=None, lead_ms=None, lead_samples=None, tail_ms=0, wav: bool = False,
                   volume=None, utterance_keys=None, sample_rate: Optional[int] = None, encoding: Optional[str] = None,
                   alignment=False, trim_db: Optional[float] = None, trim_keep_ms: Optional[float] = None,
                   loudness: Optional[float] = None, ceiling_db: Optional[float] = None,
                   limiter_ms: Optional[float] = None, true_peak: Optional[bool] = None, compression=_SESSION,
                   stretch=None, min_frames=None, target_frames=None, duration_ms=None, speakers=None, gain_db=None,
                   ramp_ms=None, pitch=None, pitch_semitones=None) -> "_native.PackedAudio":
        """The batch's finished audio as ONE contiguous stream — int16, or with ``encoding`` (else the session's
        ``output_encoding``) "ulaw" / "alaw" G.711 bytes of that int16 stream or "f32le" the float samples themselves, written by
        the packing kernel; an unknown name raises ``ValueError`` — (``mi355vits_run_packed``): only the valid
        samples of each row, rows in the order ``order`` names (default: all, in order), ``lead_ms[i]`` / ``lead_samples[i]`` of
        silence in front of entry i (``add_break``, ``tts.py:452-465``: ``int(ms / 1000 * sample_rate)`` zero samples at the
        rate of the stream: ``sample_rate``, else the session's ``output_sample_rate``, else the voice's), ``tail_ms`` after the last, with ``wav`` behind a RIFF header — one kernel, one device-to-host
        copy of exactly those bytes.  Same feed, ``volume`` and ``utterance_keys`` as ``run_pcm16``, and every entry is bitwise
        that call's row.  Returns ``_native.PackedAudio`` (``pcm``, ``rows`` — views of ``pcm`` —, ``offsets``, ``lengths``,
        ``peaks``, ``wav``, ``sample_rate``).  Always goes straight to a lane, never through the micro-batcher (``run_stream`` does).
        ``alignment`` (``True`` / ``"levels"``): sets ``PackedAudio.alignment`` (default ``None``) in STREAM coordinates — row i
        belongs to entry i and ``offsets[i]`` is added to ``start``, so ``data[start[i, t] : start[i, t] + samples[i, t]]`` is
        phoneme t of entry i in any encoding.
        ``trim_db`` (else the session's ``edge_trim_db``; ``None`` = off): each entry is its row cut to the part from the first to
        the last sample at or above ``peak * float32(10 ** (trim_db / 20))`` (``Engine.set_edge_trim``; finite and <= 0, else
        ``ValueError``) with ``int(trim_keep_ms / 1000 * rate)`` samples (else the session's ``edge_trim_keep_ms``) kept on each
        side, so ``lead_ms`` is the pause that is heard; ``PackedAudio.first`` / ``.end`` say what was kept.  The alignment of a
        trimmed stream follows the cut: a span is clipped to the entry (a phoneme wholly cut has ``samples`` = 0), the spans
        still tile the entry and sum to ``lengths[i]``; ``frames`` stay the run's own, and ``peak`` / ``rms`` stay those of the
        UNTRIMMED span.
        ``loudness`` (else the session's ``loudness_lufs``; ``None`` = off): each entry is scaled to that ITU-R BS.1770-4 integrated
        loudness in LUFS instead of to its own peak, with the gain bounded so that no sample passes ``ceiling_db`` dBFS (else the
        session's ``loudness_ceiling_db``, default -1) — ``Engine.set_loudness_target``; -70 <= loudness < 0 and a finite ceiling
        <= 0, else ``ValueError``.  ``PackedAudio.lufs`` / ``.gain`` / ``.limited`` say what was measured and applied.
        ``limiter_ms`` (else the session's ``loudness_limiter_ms``; ``None`` = off): with a loudness target, an entry the ceiling
        would hold back is brought to its target by a look-ahead peak limiter with a window of ``round(limiter_ms * rate / 1000)``
        samples instead (``Engine.set_loudness_limiter``; 1 .. 4096 samples, else ``ValueError`` naming the value); ``.gain`` is then
        the uncapped gain and ``.limited`` marks the entries the limiter acted on.
        ``true_peak`` (else the session's ``loudness_true_peak``): with a loudness target, ``ceiling_db`` bounds the entry's 4x
        oversampled peak (dBTP) instead of its largest sample, in the gain and in what the limiter looks at
        (``Engine.set_loudness_ceiling_mode``).
        ``compression`` (``"flac"`` / ``None``; else the session's ``output_compression``): the int16 stream — with everything above
        applied — as a complete FLAC file, its frames encoded on the GPU, lossless (``Engine.set_output_compression``):
        ``PackedAudio.flac`` is the file, ``.data`` / ``.rows`` / ``.wav`` are ``None``, ``.offsets`` / ``.lengths`` / ``.peaks`` /
        ``.total_samples`` are those of the uncompressed call.  ``wav=True`` with it raises ``ValueError``; any encoding but
        "s16le" is refused by the library.
        ``stretch`` / ``min_frames`` / ``target_frames`` / ``duration_ms``: timing in the same run, as for ``run_pcm16`` (a timed run
        that keeps its audio on the device, then the pack: one synchronisation more).  ``speakers``: who speaks each row, as for
        ``run_pcm16`` (likewise a run that keeps its audio on the device, then the pack).  ``gain_db`` / ``ramp_ms``: a gain per
        phoneme with ramps, as for ``run_pcm16`` (likewise); the trim, the loudness target and the limiter see the shaped waveform.
        ``pitch`` / ``pitch_semitones``: a pitch ratio per phoneme, as for ``run_pcm16`` (likewise: everything packs the warped rows)."""
        comp = self.output_compression if compression is _SESSION else _compression_name(compression)
        if comp and wav:
            raise ValueError("wav=True with compression='flac': a FLAC stream carries its own header")
        kw = self._pcm_kw(volume, utterance_keys)
        kw["_compression"] = comp
        if sample_rate is not None:
            kw["sample_rate"] = int(sample_rate)
        kw["encoding"] = _encoding_name(encoding) if encoding is not None else self.output_encoding
        rate = int(sample_rate or self.output_sample_rate or self.config.sample_rate)
        if lead_ms is not None:
            if lead_samples is not None:
                raise InvalidArgument("give lead_ms or lead_samples, not both")
            lead_samples = [int((float(ms) / 1000.0) * rate) for ms in np.asarray(lead_ms, np.float64).reshape(-1)]
        ids, lengths, sid = self._feed(input_feed, speakers is not None)
        keys = kw.pop("utterance_keys", None)
        kw.update(self._timing_kw(input_feed, stretch, min_frames, target_frames, duration_ms))
        if speakers is not None:
            kw["speakers"] = speakers
        kw.update(self._levels_kw(input_feed, gain_db, ramp_ms))
        kw.update(self._pitch_kw(input_feed, pitch, pitch_semitones))
        if alignment:
            kw["_alignment"] = _alignment_levels(alignment)
        ratio = _trim_ratio(trim_db if trim_db is not None else self.edge_trim_db)
        keep_ms = float(trim_keep_ms if trim_keep_ms is not None else self.edge_trim_keep_ms)
        if keep_ms < 0:
            raise ValueError("trim_keep_ms must be >= 0")
        kw["_trim"] = (ratio, int((keep_ms / 1000.0) * rate))
        kw["_loudness"] = _loudness_setting(loudness if loudness is not None else self.loudness_lufs,
                                            ceiling_db if ceiling_db is not None else self.loudness_ceiling_db)
        kw["_limiter"] = _native.limiter_window(limiter_ms if limiter_ms is not None else self.loudness_limiter_ms, rate)
        kw["_ceiling"] = bool(self.loudness_true_peak if true_peak is None else true_peak)
        out = self._engine_run(ids, lengths, input_feed["scales"], sid, utterance_keys=keys, _packed=True, order=order,
                               lead_samples=lead_samples, tail_samples=int((float(tail_ms) / 1000.0) * rate), wav=wav, **kw)
        if alignment:
            out, al = out
            rows = np.arange(len(out.offsets)) if order is None else np.asarray(order, np.int64).reshape(-1)
            pick = lambda a: None if a is None else a[rows]  # noqa: E731
            start, samples = al.start[rows].astype(np.int64), al.samples[rows].astype(np.int64)
            if out.first is not None:  # a trimmed stream: the spans follow the cut, clipped to the entry
                first = np.asarray(out.first, np.int64)[:, None]
                n = np.asarray(out.lengths, np.int64)[:, None]
                s0, s1 = np.clip(start - first, 0, n), np.clip(start + samples - first, 0, n)
                start, samples = s0, s1 - s0
            out.alignment = _native.Alignment(al.frames[rows], start + np.asarray(out.offsets, np.int64)[:, None],
                                              samples.astype(al.samples.dtype), pick(al.peak), pick(al.rms), al.sample_rate)
        self.last_lengths = out.lengths
        return out

    def run_stream(self, input_feed: Dict[str, np.ndarray], order=None, lead_ms=None, lead_samples=None, tail_ms=0, wav: bool = False,
                   volume=None, utterance_keys=None, sample_rate: Optional[int] = None, encoding: Optional[str] = None,
                   trim_db: Optional[float] = None, trim_keep_ms: Optional[float] = None, loudness: Optional[float] = None,
                   ceiling_db: Optional[float] = None, limiter_ms: Optional[float] = None,
                   true_peak: Optional[bool] = None, compression=None) -> "_native.PackedAudio":
        """``run_packed`` (same keywords, except ``alignment`` and ``compression``: a stream is never compressed, whatever the
        session's ``output_compression``, and ``compression="flac"`` raises ``ValueError`` — FLAC is not offered in streams yet; same ``PackedAudio``; the same bytes when ``utterance_keys`` are
        given or the noise scales are zero — a row without a key of its own takes its Philox index from its place in the shared
        call, as in any micro-batched call, so its noise is not that of the request run alone) THROUGH the micro-batcher: the
        feed's rows — one or a few sentences of one client — share an engine call with the requests of other callers that arrive
        meanwhile, and come back as that caller's own finished stream (``mi355vits_run_streams``: one stream per request, each
        with its own order, silences, header, encoding, trim and loudness target; one kernel, one device-to-host copy for the whole
        batch).  Requests group by ``sid`` presence, phoneme-length class, output rate, limiter window and ceiling mode only (the window
        and the mode are the settings ``mi355vits_run_streams`` reads from the handle, so requests with different ``limiter_ms`` or
        ``true_peak`` never share a call).  The result is a view of the
        batch's shared pinned block: nothing is copied per request.  A feed of more than ``micro_batch_max`` rows, or a session
        without a micro-batcher, takes ``run_packed`` directly."""
        if _compression_name(compression):
            raise ValueError("run_stream: FLAC is not offered in streams yet (use run_packed(..., compression='flac'))")
        ids, lengths, sid = self._feed(input_feed)
        B = int(ids.shape[0])
        if self._batcher is None or B > self._batcher._max or lengths.shape[0] != B:
            return self.run_packed(input_feed, order=order, lead_ms=lead_ms, lead_samples=lead_samples, tail_ms=tail_ms, wav=wav,
                                   volume=volume, utterance_keys=utterance_keys, sample_rate=sample_rate, encoding=encoding,
                                   trim_db=trim_db, trim_keep_ms=trim_keep_ms, loudness=loudness, ceiling_db=ceiling_db,
                                   limiter_ms=limiter_ms, true_peak=true_peak, compression=None)
        kw = self._pcm_kw(volume, utterance_keys)
        for name in ("pcm_volume", "utterance_keys"):
            if name in kw and np.ndim(kw[name]) > 0 and len(kw[name]) != B:
                raise InvalidArgument(f"per-row '{name}' must have shape [batch]")
        if sample_rate is not None:
            kw["sample_rate"] = int(sample_rate)
        rate = int(sample_rate or self.output_sample_rate or self.config.sample_rate)
        if lead_ms is not None:
            if lead_samples is not None:
                raise InvalidArgument("give lead_ms or lead_samples, not both")
            lead_samples = [int((float(ms) / 1000.0) * rate) for ms in np.asarray(lead_ms, np.float64).reshape(-1)]
        ratio = _trim_ratio(trim_db if trim_db is not None else self.edge_trim_db)
        keep_ms = float(trim_keep_ms if trim_keep_ms is not None else self.edge_trim_keep_ms)
        if keep_ms < 0:
            raise ValueError("trim_keep_ms must be >= 0")
        _check_stream_rows(order, lead_samples, B)  # against this request's own rows, before it shares a call with others
        scales = np.asarray(input_feed["scales"], np.float32)
        if scales.size not in (3, 3 * B):
            raise InvalidArgument("'scales' must hold [noise_scale, length_scale, noise_w] (or one such row per sentence)")
        kw["_kind"] = "stream"
        # a top-level keyword, not part of the stream's own settings: the micro-batcher groups by it
        kw["_limiter"] = _native.limiter_window(limiter_ms if limiter_ms is not None else self.loudness_limiter_ms, rate)
        kw["_ceiling"] = bool(self.loudness_true_peak if true_peak is None else true_peak)  # likewise
        kw["_stream"] = dict(order=order, lead_samples=lead_samples, tail_samples=int((float(tail_ms) / 1000.0) * rate), wav=bool(wav),
                             encoding=_encoding_name(encoding) if encoding is not None else self.output_encoding,
                             trim=(ratio, int((keep_ms / 1000.0) * rate)),
                             loudness=_loudness_setting(loudness if loudness is not None else self.loudness_lufs,
                                                        ceiling_db if ceiling_db is not None else self.loudness_ceiling_db))
        sid1 = None if sid is None else np.asarray(sid).reshape(-1)
        out = self._batcher.submit(np.asarray(ids, np.int64), lengths.astype(np.int64), scales, sid1, kw).result()
        self.last_lengths = out.lengths
        return out

    def run_request(self, input_feed: Dict[str, np.ndarray], order=None, lead_ms=None, lead_samples=None, tail_ms=0, wav: bool = False,
                    volume=None, utterance_keys=None, sample_rate: Optional[int] = None, encoding: Optional[str] = None,
                    trim_db: Optional[float] = None, trim_keep_ms: Optional[float] = None, loudness: Optional[float] = None,
                    ceiling_db: Optional[float] = None, limiter_ms: Optional[float] = None,
                    true_peak: Optional[bool] = None, compression=_SESSION) -> "_native.PackedAudio":
        """``run_stream`` with everything per request (``mi355vits_run_streams2``): the same keywords plus ``compression`` (``"flac"`` /
        ``None``; else the session's ``output_compression``, as ``run_packed``), THROUGH the micro-batcher.  The limiter window, the
        ceiling mode and the compression travel with the request's stream of the shared call, so requests group by ``sid`` presence,
        phoneme-length class and output rate ONLY: clients that differ in ``limiter_ms``, ``true_peak`` or ``compression`` share one
        engine call, and each still gets bitwise what ``run_packed`` gives it (with ``utterance_keys`` given or zero noise scales, as
        for ``run_stream``).  A FLAC request's ``PackedAudio.flac`` is a view of its file in the batch's shared block.  A feed of more
        than ``micro_batch_max`` rows, or a session without a micro-batcher, takes ``run_packed`` directly."""
        comp = self.output_compression if compression is _SESSION else _compression_name(compression)
        if comp and wav:
            raise ValueError("wav=True with compression='flac': a FLAC stream carries its own header")
        ids, lengths, sid = self._feed(input_feed)
        B = int(ids.shape[0])
        if self._batcher is None or B > self._batcher._max or lengths.shape[0] != B:
            return self.run_packed(input_feed, order=order, lead_ms=lead_ms, lead_samples=lead_samples, tail_ms=tail_ms, wav=wav,
                                   volume=volume, utterance_keys=utterance_keys, sample_rate=sample_rate, encoding=encoding,
                                   trim_db=trim_db, trim_keep_ms=trim_keep_ms, loudness=loudness, ceiling_db=ceiling_db,
                                   limiter_ms=limiter_ms, true_peak=true_peak, compression=comp)
        kw = self._pcm_kw(volume, utterance_keys)
        for name in ("pcm_volume", "utterance_keys"):
            if name in kw and np.ndim(kw[name]) > 0 and len(kw[name]) != B:
                raise InvalidArgument(f"per-row '{name}' must have shape [batch]")
        if sample_rate is not None:
            kw["sample_rate"] = int(sample_rate)
        rate = int(sample_rate or self.output_sample_rate or self.config.sample_rate)
        if lead_ms is not None:
            if lead_samples is not None:
                raise InvalidArgument("give lead_ms or lead_samples, not both")
            lead_samples = [int((float(ms) / 1000.0) * rate) for ms in np.asarray(lead_ms, np.float64).reshape(-1)]
        ratio = _trim_ratio(trim_db if trim_db is not None else self.edge_trim_db)
        keep_ms = float(trim_keep_ms if trim_keep_ms is not None else self.edge_trim_keep_ms)
        if keep_ms < 0:
            raise ValueError("trim_keep_ms must be >= 0")
        _check_stream_rows(order, lead_samples, B)  # against this request's own rows, before it shares a call with others
        scales = np.asarray(input_feed["scales"], np.float32)
        if scales.size not in (3, 3 * B):
            raise InvalidArgument("'scales' must hold [noise_scale, length_scale, noise_w] (or one such row per sentence)")
        kw["_kind"] = "request"  # never in one call with run_stream's requests: those read the window and the mode from the lane
        # window, mode and compression are part of the stream's own settings (mi355vits_stream_args2): nothing to group by
        kw["_stream"] = dict(order=order, lead_samples=lead_samples, tail_samples=int((float(tail_ms) / 1000.0) * rate), wav=bool(wav),
                             encoding=_encoding_name(encoding) if encoding is not None else self.output_encoding,
                             trim=(ratio, int((keep_ms / 1000.0) * rate)),
                             loudness=_loudness_setting(loudness if loudness is not None else self.loudness_lufs,
                                                        ceiling_db if ceiling_db is not None else self.loudness_ceiling_db),
                             limiter=_native.limiter_window(limiter_ms if limiter_ms is not None else self.loudness_limiter_ms, rate),
                             true_peak=bool(self.loudness_true_peak if true_peak is None else true_peak), compression=comp)
        sid1 = None if sid is None else np.asarray(sid).reshape(-1)
        out = self._batcher.submit(np.asarray(ids, np.int64), lengths.astype(np.int64), scales, sid1, kw).result()
        self.last_lengths = out.lengths
        return out

    @staticmethod
    def _pcm_kw(volume, utterance_keys) -> Dict[str, Any]:
        """``volume`` (percent, scalar or per row) and ``utterance_keys`` as the engine's keywords."""
        kw: Dict[str, Any] = {}
        if volume is not None and np.ndim(volume) > 0:
            vols = [float(v) for v in np.asarray(volume, np.float64).reshape(-1)]
            if not all(v > 0.0 for v in vols):
                raise InvalidArgument("volume must be > 0 (percent)")
            if any(v != 100.0 for v in vols):
                kw["pcm_volume"] = np.asarray([v / 100.0 for v in vols], np.float64)
        elif volume is not None and float(volume) != 100.0:
            if not float(volume) > 0.0:
                raise InvalidArgument("volume must be > 0 (percent)")
            kw["pcm_volume"] = float(volume) / 100.0
        if utterance_keys is not None:
            kw["utterance_keys"] = [int(k) for k in np.asarray(utterance_keys).reshape(-1).tolist()]
        return kw

    def _run(self, input_feed, _direct: bool = False, **kw) -> Dict[str, np.ndarray]:
        ids, lengths, sid = self._feed(input_feed)
        if self._batcher is not None and not _direct and ids.shape[0] == 1 and lengths.shape[0] == 1 and 0 <= int(lengths[0]) <= ids.shape[1]:
            sid1 = None if sid is None else np.asarray(sid).reshape(-1)
            out = self._batcher.submit(np.asarray(ids, np.int64), lengths.astype(np.int64), input_feed["scales"], sid1, kw).result()
        else:
            out = self._engine_run(ids, lengths, input_feed["scales"], sid, **kw)
        self.last_lengths = out["lengths"]
        return out

    def _feed(self, input_feed, speakers: bool = False):
        """The feed dict checked as onnxruntime checks it: (ids [B, Tx], lengths [B], sid or None).  ``speakers``: the call says
        who speaks each row itself, so a multi-speaker voice's ``sid`` may be left out."""
        if not isinstance(input_feed, dict):
            raise InvalidArgument("input_feed must be a dict of numpy arrays")
        required = ["input", "input_lengths", "scales"] + (["sid"] if self.config.is_multispeaker and not speakers else [])
        for name in required:
            if name not in input_feed:
                raise InvalidArgument(f"Required inputs ({name!r}) are missing from input feed ({list(input_feed)}).")
        for name in input_feed:
            if name not in ("input", "input_lengths", "scales", "sid"):
                raise InvalidArgument(f"Invalid input name: {name}")
        ids = np.asarray(input_feed["input"])
        if ids.ndim != 2:
            raise InvalidArgument(f"'input' must have rank 2 [batch, phonemes], got shape {ids.shape}")
        if ids.shape[1] == 0 or ids.shape[0] == 0:
            raise InvalidArgument("'input' must hold at least one phoneme id")
        if not np.issubdtype(ids.dtype, np.integer):
            raise InvalidArgument("'input' must be an int64 tensor")
        sid = input_feed.get("sid") if self.config.is_multispeaker else None
        lengths = np.asarray(input_feed["input_lengths"]).reshape(-1)
        return ids, lengths, sid

    def speaker_embedding(self, sid: int) -> np.ndarray:
        """Row ``sid`` of the voice's speaker table [gin_channels] (``mi355vits_get_speaker_embedding``; a host copy, no GPU work):
        what ``speakers=[sid]`` speaks with — average, interpolate or fit such vectors and pass the result as ``speakers``."""
        try:
            return self._engine.speaker_embedding(sid)
        except _native.NativeError as e:
            if e.code == -1:
                raise InvalidArgument(str(e)) from None
            raise RuntimeError(str(e)) from None

    def reserve_utterances(self, n: int) -> int:
        """Reserve ``n`` consecutive Philox utterance indices of this session; returns the first.  Calls without
        ``utterance_keys`` draw theirs from the same count, so reserved keys are never reused by them."""
        with self._lock:
            base = self._utterances
            self._utterances += int(n)
        return base

    def _engine_run(self, ids, lengths, scales, sid, utterance_keys=None, _packed: bool = False, sample_rate=None, encoding=None,
                    _alignment=None, _trim=None, _loudness=None, _streams=None, _limiter=0, _ceiling=False, _compression=None, **kw):
        """``_alignment`` (None, or whether levels are wanted): fetch the run's alignment on the same lane before it is released
        — a fetch after the release would race with other threads' runs — and return (result, alignment)."""
        if self._closed:
            raise RuntimeError("session is closed")
        keys = None if utterance_keys is None else list(utterance_keys)
        base = 0
        if keys is None or any(k is None for k in keys):
            base = self.reserve_utterances(ids.shape[0])
            if keys is not None:
                keys = [base + b if k is None else int(k) for b, k in enumerate(keys)]
        eng = self._free_lanes.acquire()  # blocks while every lane is busy; first come first served
        try:
            # the call owns the lane: its rate is set here and read by the engine when the run starts
            eng.set_output_rate(sample_rate if sample_rate is not None else self.output_sample_rate)
            if _packed:  # the encoding concerns packed streams only; read by the engine when the pack is planned
                eng.set_output_encoding(encoding or self.output_encoding)
                eng.set_edge_trim(*(_trim or (0.0, 0)))  # likewise; set on every call: back to off for a call that does not ask
                eng.set_loudness_target(*(_loudness or (0.0, -1.0)))  # likewise
                eng.set_output_compression(_compression)  # likewise
            if _packed or _streams is not None:  # the limiter window: set on every packed call, back to off for one that does not ask
                eng.set_loudness_limiter(_limiter or 0)
                eng.set_loudness_ceiling_mode(bool(_ceiling))  # the ceiling mode likewise: back to the sample peak for a call that does not ask
            if _streams is not None:  # every stream brings its own encoding, trim and target: of the lane's settings only the limiter window and the ceiling mode are read
                kw["streams"] = _streams
            call = eng.run_streams if _streams is not None else eng.run_packed if _packed else eng.run
            out = call(ids, lengths, scales, sid, seed=self._seed, utterance_base=base, utterance_keys=keys, **kw)
            return out if _alignment is None else (out, eng.fetch_alignment(levels=_alignment))
        except _native.NativeError as e:
            if e.code == -1:
                raise InvalidArgument(str(e)) from None
            raise RuntimeError(str(e)) from None
        finally:
            self._free_lanes.release(eng)

    @property
    def engine(self) -> _native.Engine:
        return self._engine

    def close(self) -> None:
        """Stop the micro-batch dispatcher and release every lane (weights and workspaces in HBM).  Idempotent; also
        runs when the session is garbage-collected."""
        if getattr(self, "_closed", True):
            return
        self._closed = True
        if self._batcher is not None:
            self._batcher.close()
        # wait for every call in flight: a handle is destroyed only once its lane has come back (a worker still inside
        # mi355vits_run must not find its engine freed under it)
        for _ in range(self._free_lanes.size):
            self._free_lanes.acquire()
        self._free_lanes.shutdown()  # a caller that passed the _closed check just before and queued behind us: woken with an error
        for e in reversed(self._engines):  # clones before the handles whose weights they share
            e.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
