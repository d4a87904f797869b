"""The numpy yardstick of blended speakers (include/mi355vits.h, mi355vits_run_speakers): the rule in np.float32 products and sums.

Per row the terms (sid[k], weight[k]) whose weight is not 0, in order of k:  g = fl(w_0 * e_0), then g = fl(g + fl(w_k * e_k)),
e_k = emb_g[sid[k], :].  numpy multiplies and adds float32 arrays element by element, each result rounded once: no fused
multiply-add can appear."""
import numpy as np


def mix_row(emb_g, sids, weights) -> np.ndarray:
    """g [gin] of one row.  A term of weight 0 (either sign) is skipped: its sid may hold anything."""
    emb_g = np.asarray(emb_g, np.float32)
    g = None
    for s, w in zip(np.asarray(sids).reshape(-1).tolist(), np.asarray(weights, np.float32).reshape(-1)):
        if w == 0:
            continue
        p = np.float32(w) * emb_g[int(s)]
        assert p.dtype == np.float32
        g = p if g is None else g + p
    assert g is not None, "a row whose every weight is 0"
    return g.astype(np.float32)


def mix(emb_g, sid, weight) -> np.ndarray:
    """g [B, gin] of sid / weight [B, K]."""
    return np.stack([mix_row(emb_g, s, w) for s, w in zip(np.asarray(sid), np.asarray(weight, np.float32))])


def tables(speakers):
    """sid / weight [B, K] of a list of dicts {sid: weight} and ints, padded with zero-weight terms (what the Python layer builds)."""
    rows = [list(e.items()) if isinstance(e, dict) else [(int(e), 1.0)] for e in speakers]
    K = max(len(r) for r in rows)
    sid, w = np.zeros((len(rows), K), np.int64), np.zeros((len(rows), K), np.float32)
    for b, r in enumerate(rows):
        for k, (s, x) in enumerate(r):
            sid[b, k], w[b, k] = s, x
    return sid, w
