"""Cases shared by test_output_plan.py (CPU model) and test_gpu_output_plan.py (MI355X): the one host pipeline behind every
packed-form call (Engine::run_output / finish_last_run over an OutputPlan, csrc/engine_results.cpp).  What the calls return is
tested where each feature is (test_packed_*.py, test_streams2.py, test_flac.py, ...); here is what the pipeline itself owes:

  * the launches of each call, as the profiler counts them.  LAUNCHES was recorded from the commit BEFORE the two pipelines became
    one (63f4d43), on the CPU model and on the MI355X alike: label -> calls of everything outside the synthesis graph.  Calls only:
    the bytes of the FLAC labels depend on the arithmetic of the side that ran.
  * a failing late path serves nothing afterwards;
  * the host's edge cache: a single-stream call at a ratio not held replaces it, a streams call adds to it, a held ratio launches
    nothing.

The five ragged rows of tests/test_packed_streams.py; a host pipeline has no tile size to outgrow."""
import numpy as np
import pytest

import streams2_cases as S2

from mimic3_amd._native import NativeError
from tests.test_packed_streams import FIVE, SCALES, TRIM, _inputs, _run_kw

PACK = dict(order=[2, 0, 4, 1], lead_samples=[0, 900, 1, 100], tail_samples=33)
TWO = [dict(order=[3], lead_samples=[1], wav=True, encoding="ulaw"), dict(order=[0, 3], tail_samples=5, encoding="f32le")]
HUGE = (1 << 31) - 100  # a silence that fits on its own and with no audio behind it
# label -> calls of each call, the synthesis graph's own labels left out (they are those of a plain run: checked as such)
LAUNCHES = {
    "run_packed": {"pcm16.pack": 1},
    "run_packed trimmed": {"edges": 1, "pcm16.pack": 1},
    "run_packed targeted + limited": {"limit": 1, "loudness": 1, "pcm16.pack": 1},
    "run_packed flac": {"pack.flac": 1, "pcm16.pack": 1},
    "fetch_packed": {"pcm16.pack": 1},
    "run_streams": {"pack.streams": 1},
    "run_streams measured": {"edges": 1, "loudness": 1, "pack.streams": 1},
    "run_streams2 flac": {"edges": 1, "limit": 2, "loudness": 1, "pack.flac": 1, "pack.streams": 1, "truepeak": 1, "truepeak.env": 1},
}


def _calls(eng):
    return {k: v["calls"] for k, v in eng.profile_report().items()}


def _settings(eng, trim=(0.0, 0), loudness=(None, -1.0), limiter=0):
    eng.set_edge_trim(*trim)
    eng.set_loudness_target(*loudness)
    eng.set_loudness_limiter(limiter)


def observe_launches(eng, cfg):
    """label -> calls of each call of LAUNCHES on a fresh engine: (the calls' own labels, whether the rest was a plain run's)."""
    ids, lens = _inputs(cfg)
    args = (ids, lens, SCALES, None)
    eng.profile_enable(True)
    eng.profile_reset()
    eng.run(*args, **_run_kw())
    graph = _calls(eng)
    seen, graph_same = {}, {}

    def note(name, call, run=True):
        eng.profile_reset()
        call()
        rep = _calls(eng)
        seen[name] = {k: c for k, c in rep.items() if k not in graph}
        graph_same[name] = {k: c for k, c in rep.items() if k in graph} == (graph if run else {})

    try:
        note("run_packed", lambda: eng.run_packed(*args, wav=True, **PACK, **_run_kw()))
        _settings(eng, trim=TRIM)
        note("run_packed trimmed", lambda: eng.run_packed(*args, **PACK, **_run_kw()))
        _settings(eng, loudness=S2.TARGET, limiter=32)
        note("run_packed targeted + limited", lambda: eng.run_packed(*args, **PACK, **_run_kw()))
        _settings(eng)
        note("run_packed flac", lambda: eng.run_packed(*args, compression="flac", **PACK, **_run_kw()))
        note("fetch_packed", lambda: eng.fetch_packed(wav=True, **PACK), run=False)
        note("run_streams", lambda: eng.run_streams(*args, streams=TWO, **_run_kw()))
        note("run_streams measured", lambda: eng.run_streams(*args, streams=FIVE, **_run_kw()))
        note("run_streams2 flac", lambda: eng.run_streams(*args, streams=S2.SEVEN, **_run_kw()))
    finally:
        _settings(eng)
        eng.profile_enable(False)
    return seen, graph_same


def check_launches(eng, cfg):
    seen, graph_same = observe_launches(eng, cfg)
    print("launches:", seen)
    assert seen == LAUNCHES
    assert all(graph_same.values()), graph_same


def check_failing_late_path_serves_nothing(eng, cfg):
    """A limit the trimmed sizes exceed is found after the synthesis: neither that run nor the one before it is served."""
    ids, lens = _inputs(cfg)
    args = (ids, lens, SCALES, None)
    late = [
        lambda: eng.run_packed(*args, order=[1], lead_samples=[HUGE], **_run_kw()),
        lambda: eng.run_streams(*args, streams=[dict(order=[0]), dict(order=[1], lead_samples=[HUGE], trim=TRIM)], **_run_kw()),
    ]
    texts = ["pack entry 0: total_samples exceeds 2^31 - 1", "stream 1: pack entry 0: total_samples exceeds 2^31 - 1"]
    try:
        for k, (call, text) in enumerate(zip(late, texts)):
            _settings(eng)
            eng.run(*args, **_run_kw())
            assert eng.fetch_packed().total_samples > 0  # the run before is served until the failing call starts
            _settings(eng, trim=TRIM if k == 0 else (0.0, 0))  # (the streams call brings its own trim)
            with pytest.raises(NativeError) as e:
                call()
            assert e.value.code == -1 and str(e.value).endswith(text), str(e.value)
            _settings(eng)
            with pytest.raises(NativeError, match="fetch_packed: no completed run on this handle"):
                eng.fetch_packed()
            with pytest.raises(NativeError, match="fetch_streams: no completed run on this handle"):
                eng.fetch_streams(TWO)
    finally:
        _settings(eng)


def check_edge_cache(eng, cfg):
    ids, lens = _inputs(cfg)
    r1, r2, r3 = (float(np.float32(r)) for r in (0.5, 0.25, 0.125))
    eng.profile_enable(True)

    def edges_launched(call):
        eng.profile_reset()
        got = call()
        return _calls(eng).get("edges", 0), got

    def fetch_edges_at(ratio):
        eng.set_edge_trim(ratio, 3)
        return edges_launched(eng.fetch_edges)

    try:
        eng.run(ids, lens, SCALES, None, **_run_kw())
        n, first = fetch_edges_at(r1)
        assert n == 1
        # a streams call at new ratios ADDS to what the host holds: one k_edges per distinct ratio not held, r1 stays
        streams = [dict(order=[0], trim=(r2, 3)), dict(order=[1, 0], trim=(r1, 3)), dict(order=[2], trim=(r2, 0))]
        n, got = edges_launched(lambda: eng.fetch_streams(streams))
        assert n == 1
        assert edges_launched(lambda: eng.fetch_streams(streams))[0] == 0  # every ratio held: nothing launched
        n, again = fetch_edges_at(r1)
        assert n == 0 and np.array_equal(again.first, first.first) and np.array_equal(again.end, first.end)
        n, at_r2 = fetch_edges_at(r2)
        assert n == 0 and int(got[0].first[0]) == int(at_r2.first[0]) and int(got[0].end[0]) == int(at_r2.end[0])
        # a single-stream call at a ratio not held REPLACES it
        eng.set_edge_trim(r3, 3)
        n, pk = edges_launched(lambda: eng.fetch_packed(order=[0, 1]))
        assert n == 1
        n, pk2 = edges_launched(lambda: eng.fetch_packed(order=[0, 1]))  # held now
        assert n == 0 and pk2.data.tobytes() == pk.data.tobytes()
        n, back = fetch_edges_at(r1)
        assert n == 1 and np.array_equal(back.first, first.first) and np.array_equal(back.end, first.end)
        assert fetch_edges_at(r3)[0] == 1  # ... as fetch_edges itself does
    finally:
        _settings(eng)
        eng.profile_enable(False)
