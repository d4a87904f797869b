"""Blended and caller-supplied speakers per row (mi355vits_run_speakers, k_speaker_cond_mix) on the CPU model of the kernels;
test_gpu_speaker_mix.py runs the same checks on the MI355X.

The yardstick is tests/speaker_ref.py: the blend in np.float32 products and sums.  Everything is compared bit for bit — g against the
yardstick, the projections against k_speaker_cond on a table that carries g as a row, a whole run against the plain run on a voice
whose emb_g carries g as its last row: the rule has no tolerance.  Only the comparison with the CPU oracle uses the project's own
tests/util.parity_tol."""
import ctypes

import numpy as np
import pytest

from mimic3_amd import weights as W
from mimic3_amd._native import Engine, NativeError, Result, SpeakerArgs, WANT_FLOAT, WANT_PCM16
from mimic3_amd.config import VitsConfig
from mimic3_amd.session import InferenceSession, SessionOptions
from tests import speaker_ref as SR
from tests.detdp_util import DetOracle, det_config
from tests.test_timing import KEYS, LENS, SCALES, SEED, feed, same_run

POISON = np.float32(-7.5e29)
# a kernel-alone case: (gin, B, K, Cout of every consumer in one job table; a consumer named in `nobias` has a NULL bias)
KERNEL_CASES = [
    dict(gin=1, B=1, K=1, couts=(1,), nobias=(0,)),
    dict(gin=16, B=2, K=2, couts=(3, 4, 5), nobias=()),
    dict(gin=63, B=5, K=8, couts=(5, 1, 192), nobias=(1,)),
    dict(gin=64, B=33, K=2, couts=(4, 3), nobias=()),
    dict(gin=65, B=5, K=1, couts=(192, 5), nobias=(0,)),
    dict(gin=512, B=33, K=8, couts=(5, 1536, 1, 3), nobias=(3,)),
    dict(gin=512, B=2, K=2, couts=(1, 3, 4, 5, 192, 4, 3, 1, 5, 4), nobias=(2, 9)),  # a full job table
]
# a gin beyond the register slices (the kernel walks the weight row per row, and the row block shrinks): not in the issue's list
# and one row more than the kernel's row block
KERNEL_CASES_WIDE = [dict(gin=513, B=33, K=2, couts=(5, 17), nobias=(1,)), dict(gin=8192, B=3, K=1, couts=(3,), nobias=()),
                     dict(gin=16, B=9, K=8, couts=(4, 17), nobias=())]


def planted_table(rng, S, gin):
    """emb_g of synthetic_weights' range (normal) with a few -0.0 and exact integers planted."""
    e = rng.standard_normal((S, gin)).astype(np.float32)
    flat = e.reshape(-1)
    at = rng.permutation(flat.size)[:6]
    for i, v in zip(at, (-0.0, -0.0, 3.0, -2.0, 0.0, 1.0)):
        flat[i] = np.float32(v)
    return e


def planted_mix(rng, B, K, S):
    """sid / weight [B, K]: 1.0, 0.0 (skipped; in position 0 too, with a sid outside the table), negatives, 1.5 / -0.5, a duplicated
    sid; every row keeps a term."""
    sid = rng.integers(0, S, (B, K)).astype(np.int64)
    w = rng.uniform(-1.0, 1.0, (B, K)).astype(np.float32)
    for b in range(B):
        kind = b % 6
        if kind == 0:
            w[b, 0] = 1.0
            w[b, 1:] = 0.0  # the table row itself
        elif kind == 1 and K > 1:
            w[b, 0], sid[b, 0] = 0.0, S + 1000  # skipped in position 0: its sid is never looked at
        elif kind == 2 and K > 1:
            w[b, 0], w[b, 1] = 1.5, -0.5
            w[b, 2:] = 0.0
        elif kind == 3 and K > 1:
            sid[b, 1] = sid[b, 0]  # a duplicated sid
        elif kind == 4 and K > 2:
            w[b, 1] = -0.0  # minus zero is zero: skipped
            sid[b, 1] = -5
    return sid, w


def kernel_case(c, seed=0):
    rng = np.random.default_rng(1000 * seed + 7 * c["gin"] + c["B"])
    S = 7
    emb = planted_table(rng, S, c["gin"])
    sid, w = planted_mix(rng, c["B"], c["K"], S)
    cons = [(rng.standard_normal((co, c["gin"])).astype(np.float32), None if q in c["nobias"] else rng.standard_normal(co).astype(np.float32))
            for q, co in enumerate(c["couts"])]
    return emb, sid, w, cons


def check_kernel_alone(lib, c):
    """Contract 1 (the hook's g is the yardstick's, bitwise) and contract 2 (every consumer's output is bitwise k_speaker_cond's on a
    table that carries g as extra rows); the floats behind every output keep the poison."""
    emb, sid, w, cons = kernel_case(c)
    B, gin, S = c["B"], c["gin"], emb.shape[0]
    want_g = SR.mix(emb, sid, w)
    aug = np.concatenate([emb, want_g])  # row S + b = g of row b
    for mode in ("mix", "vectors"):
        if mode == "mix":
            g, outs = lib.test_speaker_cond_mix(cons, emb_g=emb, sid=sid, weight=w)
        else:
            g, outs = lib.test_speaker_cond_mix(cons, vectors=want_g)
        assert g[: B * gin].tobytes() == want_g.tobytes(), (c, mode, np.argwhere(g[: B * gin].reshape(B, gin) != want_g)[:4].tolist())
        assert (g[B * gin:] == POISON).all()
        for q, (cw, cb) in enumerate(cons):
            ref = lib.test_speaker_cond(aug, S + np.arange(B), cw, cb)
            n = B * cw.shape[0]
            assert (ref[n:] == POISON).all() and not (ref[:n] == POISON).any()
            assert outs[q][:n].tobytes() == ref[:n].tobytes(), (c, mode, q, np.argwhere(outs[q][:n] != ref[:n])[:4].tolist())
            assert (outs[q][n:] == POISON).all(), (c, mode, q)
    # a one-term mix of weight 1.0 is the table row, -0.0 included
    one_s = np.arange(B, dtype=np.int64).reshape(B, 1) % S
    g, _ = lib.test_speaker_cond_mix(cons[:1], emb_g=emb, sid=one_s, weight=np.ones((B, 1), np.float32))
    assert g[: B * gin].tobytes() == emb[one_s[:, 0]].tobytes()


@pytest.mark.parametrize("c", KERNEL_CASES + KERNEL_CASES_WIDE, ids=lambda c: "gin%d-B%d-K%d-%djobs" % (c["gin"], c["B"], c["K"], len(c["couts"])))
def test_kernel_alone_matches_the_yardstick_and_k_speaker_cond(emu_lib, c):
    check_kernel_alone(emu_lib, c)


def test_the_yardstick_on_rows_worked_by_hand():
    e = np.array([[1.0, -0.0, 3.0], [0.5, 2.0, -1.0]], np.float32)
    assert SR.mix_row(e, [0], [1.0]).tobytes() == e[0].tobytes()  # -0.0 stays -0.0
    assert SR.mix_row(e, [99, 1], [0.0, 1.0]).tobytes() == e[1].tobytes()  # the skipped term's sid is never looked at
    assert SR.mix_row(e, [0, 1], [1.5, -0.5]).tolist() == [1.25, -1.0, 5.0]
    # single roundings: fl(fl(0.1 * 3) + fl(0.7 * -1)), not the exactly-rounded sum of products
    g = SR.mix_row(e, [0, 1], [0.1, 0.7])
    assert g[2] == np.float32(np.float32(0.1) * np.float32(3.0)) + np.float32(np.float32(0.7) * np.float32(-1.0))
    sid, w = SR.tables([2, {0: 0.7, 1: 0.3}])
    assert sid.tolist() == [[2, 0], [0, 1]] and w.tolist() == [[1.0, 0.0], [np.float32(0.7), np.float32(0.3)]]
    with pytest.raises(AssertionError):
        SR.mix_row(e, [0, 1], [0.0, -0.0])


# ------------------------------------------------------------------------------------------ through the engine
N_SPK = 3
MIXES = [{0: 0.7, 2: 0.3}, 1, {2: 1.5, 0: -0.5}, {1: 0.25, 1000: 0.0, 0: -0.75, 2: 1.0}, {0: 0.5, 1: 0.5}]  # B = 5, every row another mix


def voice(kind, seed=31):
    """(cfg, weights) of a multi-speaker voice with -0.0 and exact integers planted in emb_g."""
    cfg = {"tiny": lambda: VitsConfig.tiny(n_speakers=N_SPK), "h192": lambda: VitsConfig.tiny_h192(n_speakers=N_SPK),
           "det": lambda: det_config(VitsConfig.tiny(n_speakers=N_SPK), 64)}[kind]()
    w = W.synthetic_weights(cfg, seed=seed, frames_per_id=3.0)
    e = w["emb_g.weight"]
    e[0, 1], e[2, 3], e[1, 0], e[0, 5] = -0.0, -0.0, 2.0, -1.0
    return cfg, w


def augmented(cfg, w, g):
    """(cfg, blob) of the same voice with the rows of g [n, gin] appended to emb_g: speakers n_speakers .. n_speakers + n - 1."""
    c2 = VitsConfig(**{**cfg.__dict__})
    c2.n_speakers = cfg.n_speakers + len(g)
    w2 = dict(w)
    w2["emb_g.weight"] = np.concatenate([w["emb_g.weight"], np.asarray(g, np.float32)]).astype(np.float32)
    return c2, W.pack(c2, w2), w2


def run(eng, a, rows=slice(None), sid=None, **kw):
    if "speakers" in kw and not isinstance(kw["speakers"], SpeakerArgs):
        kw["speakers"] = list(kw["speakers"])[rows] if isinstance(rows, slice) else [kw["speakers"][rows]]
    keys = KEYS[rows] if isinstance(rows, slice) else [KEYS[rows]]
    out = eng.run(a["ids"][rows], a["lens"][rows], SCALES, None if sid is None else np.asarray(sid)[rows], seed=SEED, utterance_keys=keys,
                  want_float=True, want_pcm16=True, **kw)
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in out.items()}


def calls(eng):
    return {k: v["calls"] for k, v in eng.profile_report().items()}


def run_speakers_raw(eng, a, spk, sid=None, flags=WANT_FLOAT | WANT_PCM16):
    """mi355vits_run_speakers itself with `spk` = None (NULL) or a SpeakerArgs."""
    args, rows, per_row, keep = eng._args(a["ids"], a["lens"], SCALES, sid, SEED, 0, None, None, None, 1.0, KEYS[: len(a["lens"])])
    args.flags = flags
    r = Result()
    rc = eng.native.lib.mi355vits_run_speakers(eng._h, ctypes.byref(args), ctypes.byref(rows) if per_row else None, None,
                                               None if spk is None else ctypes.byref(spk), ctypes.byref(r))
    if rc != 0:
        eng._check(rc)
    out = eng._take(r)
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in out.items()}


def check_whole_run(make, cfg, w, a, mixes, oracle_row=None, oracle=None):
    """Contracts 1 and 3: the "g" tap is the yardstick's g, and the mixed run is bitwise the plain run with sid = n_speakers + b on the
    voice whose emb_g carries the blended vectors as further rows.  One row against the CPU oracle on the augmented weights."""
    B = len(mixes)
    sid, wt = SR.tables(mixes)
    g = SR.mix(w["emb_g.weight"], sid, wt)
    eng = make(W.pack(cfg, w))
    mixed = run(eng, a, speakers=mixes, debug_taps=True)
    tap = eng.tap("g")
    assert tap.shape == (B, cfg.gin_channels, 1) and tap[:, :, 0].tobytes() == g.tobytes()
    cfg2, blob2, w2 = augmented(cfg, w, g)
    eng2 = make(blob2)
    plain = run(eng2, a, sid=cfg.n_speakers + np.arange(B))
    same_run(mixed, plain)
    if oracle_row is not None:
        from tests.util import parity_tol, rel_rms

        b = oracle_row
        ora = oracle(cfg2, w2)
        L = int(a["lens"][b])
        o = ora.infer(a["ids"][b:b + 1, :L], a["lens"][b:b + 1], (0.0, 1.0, 0.0), sid=np.array([cfg.n_speakers + b]))
        one = eng.run(a["ids"][b:b + 1, :L], a["lens"][b:b + 1], (0.0, 1.0, 0.0), None, speakers=[mixes[b]], want_float=True)
        n = int(one["lengths"][0])
        assert n == int(o["audio_lengths"][0])
        assert rel_rms(one["audio"][0, :n], o["audio"][0, 0, :n]) < parity_tol(eng)
    eng2.close()
    return eng, mixed, g


def check_identities(eng, make_same, a, mixes, mixed, g):
    """Contract 4: {s: 1.0} and a vector equal to speaker_embedding(s) are the plain sid run; a vector equal to the yardstick's mix is
    the mix run; a row of a batch is the row alone; permuting the rows permutes the results."""
    B = len(mixes)
    sids = a["sid"]
    plain = run(eng, a, sid=sids)
    same_run(run(eng, a, speakers=[{int(s): 1.0} for s in sids]), plain)
    same_run(run(eng, a, speakers=[int(s) for s in sids]), plain)
    emb = [eng.speaker_embedding(int(s)) for s in sids]
    same_run(run(eng, a, speakers=emb), plain)
    same_run(run(eng, a, speakers=list(g)), mixed)
    for b in (0, 3):
        e1 = make_same()
        one = run(e1, a, rows=slice(b, b + 1), speakers=mixes)
        n = int(mixed["lengths"][b])
        assert int(one["lengths"][0]) == n and one["peaks"].tobytes() == mixed["peaks"][b:b + 1].tobytes()
        assert one["audio"][0, :n].tobytes() == mixed["audio"][b, :n].tobytes() and one["pcm"][0, :n].tobytes() == mixed["pcm"][b, :n].tobytes()
        e1.close()
    perm = [3, 0, 4, 1, 2][:B]
    pa = dict(ids=a["ids"][perm], lens=a["lens"][perm], sid=None)
    out = eng.run(pa["ids"], pa["lens"], SCALES, None, seed=SEED, utterance_keys=[KEYS[p] for p in perm], want_float=True, want_pcm16=True,
                  speakers=[mixes[p] for p in perm])
    for i, p in enumerate(perm):
        n = int(mixed["lengths"][p])
        assert int(out["lengths"][i]) == n and out["audio"][i, :n].tobytes() == mixed["audio"][p, :n].tobytes()
        assert out["pcm"][i, :n].tobytes() == mixed["pcm"][p, :n].tobytes() and out["peaks"][i] == mixed["peaks"][p]


def check_composes(eng, eng_aug, cfg, a, mixes):
    """Contract 5: target_frames with speakers; a DEVICE_ONLY speakers run + fetch_packed / fetch_alignment equals the forms of the
    augmented-voice run; speakers=None leaves the launch list of the multi-speaker run what it is without the feature."""
    B = len(mixes)
    aug_sid = cfg.n_speakers + np.arange(B)
    target = np.array([90, 7, 60, 120, 33][:B], np.int32)
    out = run(eng, a, speakers=mixes, target_frames=target)
    assert np.array_equal(out["lengths"], target.astype(np.int64) * cfg.hop_length)
    assert np.array_equal(eng.fetch_alignment().frames.sum(axis=1), target)
    same_run(out, run(eng_aug, a, sid=aug_sid, target_frames=target))
    # output forms
    kw = dict(order=[3, 0, 4, 1, 2][:B], lead_samples=[5, 0, 9, 1, 2][:B], wav=True)
    eng.run(a["ids"], a["lens"], SCALES, None, seed=SEED, utterance_keys=KEYS[:B], want_float=False, device_only=True, speakers=mixes)
    pk, al = eng.fetch_packed(**kw), eng.fetch_alignment(levels=True)
    eng_aug.run(a["ids"], a["lens"], SCALES, aug_sid, seed=SEED, utterance_keys=KEYS[:B], want_float=False, device_only=True)
    pk2, al2 = eng_aug.fetch_packed(**kw), eng_aug.fetch_alignment(levels=True)
    assert pk.data.tobytes() == pk2.data.tobytes() and np.asarray(pk.wav).tobytes() == np.asarray(pk2.wav).tobytes()
    assert np.array_equal(pk.offsets, pk2.offsets) and np.array_equal(pk.lengths, pk2.lengths)
    for x, y in ((al.frames, al2.frames), (al.start, al2.start), (al.samples, al2.samples), (al.peak, al2.peak), (al.rms, al2.rms)):
        assert x.tobytes() == y.tobytes()
    pk3 = eng.run_packed(a["ids"], a["lens"], SCALES, None, seed=SEED, utterance_keys=KEYS[:B], speakers=mixes, **kw)
    assert pk3.data.tobytes() == pk.data.tobytes()
    # the launch lists
    eng.profile_enable(True)
    eng.profile_reset()
    plain = run(eng, a, sid=a["sid"])
    want = calls(eng)
    assert want["speaker_cond"] == 1 and "speaker_cond.mix" not in want
    eng.profile_reset()
    same_run(run_speakers_raw(eng, a, None, sid=a["sid"]), plain)  # speakers == NULL: the call is run_timed
    assert calls(eng) == want
    eng.profile_reset()
    run(eng, a, speakers=mixes)
    got = calls(eng)
    assert got.pop("speaker_cond.mix") == 1 and got == {k: v for k, v in want.items() if k != "speaker_cond"}
    eng.profile_enable(False)


def check_errors(eng, single, a):
    """Contract 6: every refusal is MI355VITS_ERR_INVALID, names the row, comes before anything is launched and leaves the previous
    run served."""
    B = len(a["lens"])
    gin = eng.config.gin_channels
    kept = run(eng, a, sid=a["sid"])
    served = lambda: same_run({**eng.fetch(want_float=True, want_pcm16=True)}, kept)  # noqa: E731

    def refused(match, spk):
        with pytest.raises(NativeError, match=match) as err:
            run(eng, a, speakers=spk) if not isinstance(spk, SpeakerArgs) else run_speakers_raw(eng, a, spk)
        assert err.value.code == -1
        served()

    ok = [{0: 0.5, 1: 0.5}] * B
    refused("row 2, term 1: speaker id 3 out of range", ok[:2] + [{0: 0.5, N_SPK: 0.5}] + ok[3:])
    refused("row 4, term 0: speaker id -1 out of range", ok[:4] + [{-1: 1.0}])
    refused("row 1, term 0: speaker weight must be finite", ok[:1] + [{0: np.nan}] + ok[2:])
    refused("row 1, term 1: speaker weight must be finite", ok[:1] + [{0: 1.0, 1: np.inf}] + ok[2:])
    refused("row 3, term 0: speaker weight must be finite and within -1024 .. 1024", ok[:3] + [{2: 1024.5}] + ok[4:])
    run(eng, a, speakers=ok[:3] + [{2: -1024.0}] + ok[4:])  # the bound itself is served
    kept = run(eng, a, sid=a["sid"])
    refused("row 2: every speaker weight is 0", ok[:2] + [{0: 0.0, 1: -0.0}] + ok[3:])
    vec = np.stack([eng.speaker_embedding(0)] * B)
    bad = vec.copy()
    bad[3, 7] = np.inf
    refused("row 3: speaker vector must be finite", list(bad))
    bad[3, 7] = np.nan
    refused("row 3: speaker vector must be finite", list(bad))
    sid, wt = SR.tables(ok)
    i64p, f32p = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_float)

    def sa(n_terms=0, mix=False, vectors=False, **kw):
        s = SpeakerArgs()
        s.n_terms = n_terms
        if mix:
            s.mix_sid, s.mix_weight = sid.ctypes.data_as(i64p), wt.ctypes.data_as(f32p)
        if vectors:
            s.vectors = vec.ctypes.data_as(f32p)
        return s

    refused("mix_sid / mix_weight and vectors exclude each other", sa(2, mix=True, vectors=True))
    refused("give mix_sid and mix_weight, or vectors", sa(2))
    refused("n_terms must be within 1 .. 8", sa(0, mix=True))
    refused("n_terms must be within 1 .. 8", sa(9, mix=True))
    refused("n_terms must be 0 with vectors", sa(1, vectors=True))
    half = sa(2)
    half.mix_sid = sid.ctypes.data_as(i64p)
    refused("mix_sid and mix_weight go together", half)
    res = sa(2, mix=True)
    res.reserved[5] = 1
    refused("speakers: reserved fields must be 0", res)
    same_run(run_speakers_raw(eng, a, sa(2, mix=True)), run(eng, a, speakers=ok))  # the struct built by hand is served
    kept = run(eng, a, sid=a["sid"])
    # the Python layer's own refusals
    for spk in (ok[:-1], ok[:-1] + [vec[0]], [vec[0][:-1]] * B, [{s: 0.1 for s in range(9)}] * B):
        with pytest.raises(ValueError):
            run(eng, a, speakers=spk)
        served()
    # the table rows
    with pytest.raises(NativeError, match="speaker id 3 out of range") as err:
        eng.speaker_embedding(N_SPK)
    assert err.value.code == -1
    with pytest.raises(NativeError, match="out of range"):
        eng.speaker_embedding(-1)
    out = np.zeros(gin, np.float32)
    rc = eng.native.lib.mi355vits_get_speaker_embedding(eng._h, 0, out.ctypes.data_as(f32p), gin - 1)
    assert rc == -1 and not out.any()
    served()
    # a single-speaker voice
    a1 = dict(ids=a["ids"], lens=a["lens"], sid=None)
    kept1 = run(single, a1)
    with pytest.raises(NativeError, match="voice has no speaker embedding") as err:
        run(single, a1, speakers=[0] * B)
    assert err.value.code == -1
    same_run({**single.fetch(want_float=True, want_pcm16=True)}, kept1)
    with pytest.raises(NativeError, match="voice has no speaker embedding"):
        single.speaker_embedding(0)


@pytest.fixture(scope="module")
def voices(emu_lib):
    made = {}

    def get(kind):
        if kind not in made:
            cfg, w = voice(kind)
            a = feed(cfg)
            eng, mixed, g = check_whole_run(lambda blob: Engine(blob, library=emu_lib), cfg, w, a, MIXES, oracle_row=2 if kind != "h192" else None,
                                            oracle=oracle_for(kind))
            made[kind] = (cfg, w, a, eng, mixed, g)
        return made[kind]

    yield get
    for v in made.values():
        v[3].close()


def oracle_for(kind):
    from oracle.vits_oracle import VitsOracle

    return DetOracle if kind == "det" else VitsOracle


@pytest.mark.parametrize("kind", ["tiny", "h192", "det"])
def test_a_mixed_run_is_the_plain_run_on_the_augmented_voice(voices, kind):
    voices(kind)  # check_whole_run: the g tap, bitwise equality with the augmented voice, one row against the CPU oracle


@pytest.mark.parametrize("kind", ["tiny", "det"])
def test_identities_rows_alone_and_permutation(emu_lib, voices, kind):
    cfg, w, a, eng, mixed, g = voices(kind)
    blob = W.pack(cfg, w)
    check_identities(eng, lambda: Engine(blob, library=emu_lib), a, MIXES, mixed, g)


def test_composes_with_timing_output_forms_and_the_launch_list(emu_lib, voices):
    cfg, w, a, eng, mixed, g = voices("tiny")
    eng_aug = Engine(augmented(cfg, w, g)[1], library=emu_lib)
    check_composes(eng, eng_aug, cfg, a, MIXES)
    eng_aug.close()


def test_errors(emu_lib, voices):
    cfg, w, a, eng, mixed, g = voices("tiny")
    c1 = VitsConfig.tiny()
    single = Engine(W.pack(c1, W.synthetic_weights(c1, seed=31, frames_per_id=3.0)), library=emu_lib)
    check_errors(eng, single, a)
    single.close()


def test_session_keywords(emu_lib):
    """run_pcm16 / run_packed(speakers=) and speaker_embedding: ints and dicts mixed in one call, vectors in a call of their own, the
    feed's sid optional; such a call goes straight to a lane, never through the micro-batcher."""
    cfg, w = voice("tiny")
    so = SessionOptions()
    so.seed = SEED
    so.micro_batch_window_ms = 200.0
    sess = InferenceSession(W.pack(cfg, w), sess_options=so, _library=emu_lib)
    a = feed(cfg, lens=LENS[:3])
    fd = {"input": a["ids"], "input_lengths": a["lens"], "scales": SCALES}
    batches = []
    sess._batcher.submit, submit = (lambda *x, **k: batches.append(1) or submit(*x, **k)), sess._batcher.submit
    spk = [1, {0: 0.7, 2: 0.3}, {2: 1.0}]
    rows, lengths = sess.run_pcm16(fd, utterance_keys=KEYS[:3], speakers=spk)
    assert not batches
    plain, _ = sess.run_pcm16({**fd, "sid": np.array([1, 0, 2])}, utterance_keys=KEYS[:3])
    assert rows[0].tobytes() == plain[0].tobytes() and rows[2].tobytes() == plain[2].tobytes() and rows[1].tobytes() != plain[1].tobytes()
    g = SR.mix(w["emb_g.weight"], *SR.tables(spk))
    assert sess.speaker_embedding(2).tobytes() == w["emb_g.weight"][2].tobytes()
    rows2, _ = sess.run_pcm16({**fd, "sid": np.array([0, 0, 0])}, utterance_keys=KEYS[:3], speakers=list(g))  # a sid in the feed is not read
    assert all(x.tobytes() == y.tobytes() for x, y in zip(rows, rows2))
    pk = sess.run_packed(fd, utterance_keys=KEYS[:3], speakers=spk, order=[2, 0])
    assert pk.rows[0].tobytes() == rows[2].tobytes() and pk.rows[1].tobytes() == rows[0].tobytes()
    rows3, lengths3 = sess.run_pcm16(fd, utterance_keys=KEYS[:3], speakers=spk, duration_ms=[60.0, None, None])
    assert int(lengths3[0]) == 165 * cfg.hop_length and rows3[2].tobytes() == rows[2].tobytes()
    with pytest.raises(ValueError, match="calls of their own"):
        sess.run_pcm16(fd, speakers=[1, g[1], 2])
    with pytest.raises(ValueError, match="one entry per row"):
        sess.run_pcm16(fd, speakers=[1, 2])
    from mimic3_amd.session import InvalidArgument

    with pytest.raises(InvalidArgument, match="row 1, term 0: speaker id 7 out of range"):
        sess.run_pcm16(fd, speakers=[1, 7, 2])
    with pytest.raises(InvalidArgument, match="sid"):
        sess.run_pcm16(fd)  # without speakers the feed's sid is required as before
    with pytest.raises(InvalidArgument, match="out of range"):
        sess.speaker_embedding(3)
    sess.close()


def test_plain_c99_client(emu_lib, tmp_path):
    """tests/abi/abi_speaker_client.c: the new struct and entry points are C99; a one-term mix, a vector from
    mi355vits_get_speaker_embedding and two refusals hold from C."""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "abi_speaker_client"
    libdir, libname = os.path.split(emu_lib.path)
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                    os.path.join(root, "tests", "abi", "abi_speaker_client.c"), "-o", str(exe), "-L", libdir,
                    "-l:" + libname, "-Wl,-rpath," + libdir], check=True)
    cfg = VitsConfig.tiny(n_speakers=N_SPK)
    W.save(str(tmp_path / "voice.m355"), cfg, W.synthetic_weights(cfg, seed=17))
    p = subprocess.run([str(exe), str(tmp_path / "voice.m355")], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "expected failure rc=-1 msg=row 1, term 1: speaker id 3 out of range (the voice has 3 speakers)" in p.stdout
    assert "expected failure rc=-1 msg=row 0: every speaker weight is 0" in p.stdout
    assert "expected failure rc=-1 msg=capacity of 15 floats is below gin_channels = 16" in p.stdout
    assert "speakers ok" in p.stdout
