"""Host statement of relation negatives (include/emgraph_hip.h: emg_relneg_forward / emg_relneg_backward).  numpy only;
the draw is restated on the Philox restatement of tests/_negsample_ref.py.

Draw j of positive i = (s, p, o) is (s, p', o):  idx = emg_corrupt_codes' own draw over n_rel - 1 choices (side forced, keep bit zero)
at draw index j * B + i under counter counter0 + sd_p;  p' = idx + (idx >= p).  Slot order of a step: the entity sides in the order
given, then 'p'."""
import numpy as np

from tests import _negsample_ref as ns
from tests import _shared_ref as sh

TRANSE_L1, TRANSE_L2, DISTMULT, COMPLEX, HOLE, TRANSE_P, ROTATE = range(7)
SIMPLE = 8


def canonical_sides(sides):
    sides = [sides] if isinstance(sides, str) else list(sides)
    return [s for s in sides if s != "p"] + ["p"] * sides.count("p")


def draw_idx(B, eta, n_rel, seed, counter):
    """codes_p [eta * B] (int64): entry j * B + i = idx in [0, n_rel - 1)"""
    words = ns.attempt_words(seed, counter, np.arange(int(B) * int(eta), dtype=np.uint64), 0)
    return np.array(ns.attempt_index(words, int(n_rel) - 1), dtype=np.int64)


def shift(idx, p):
    """p' of the draws ``idx`` [eta * B] for the positives' relations ``p`` [B]"""
    idx, p = np.asarray(idx, dtype=np.int64), np.asarray(p, dtype=np.int64)
    pt = np.tile(p, len(idx) // len(p))
    return idx + (idx >= pt)


def negatives(pos, idx):
    """[eta * B, 3] triples (row j * B + i)"""
    pos = np.asarray(pos, dtype=np.int64)
    B = len(pos)
    i = np.tile(np.arange(B), len(idx) // B)
    return np.stack([pos[i, 0], shift(idx, pos[:, 1]), pos[i, 2]], 1)


def triple_grads(model, a, p, b, g, scale):
    """d(sum g * f)/d(a, p, b), float64 rows: tests/_shared_ref.py's for its seven models, SimplE here
    (f = scale * sum_c a[c] p[c] swap(b)[c] over rows [h | t], [r | r_inv])"""
    if model != SIMPLE:
        return sh.triple_grads(model, a, p, b, g, scale)
    n = a.shape[1] // 2
    sw = lambda x: np.concatenate([x[:, n:], x[:, :n]], 1)  # noqa: E731
    w = (g * scale)[:, None]
    return w * p * sw(b), w * a * sw(b), sw(w * p * a)


def dense_grads(model, E, R, trip, g, scale):
    """(dE, dR) float64: the gradient rows of the triples ``trip`` [n, 3] under dL/dscore ``g`` [n], added up by destination"""
    E64, R64 = np.asarray(E, dtype=np.float64), np.asarray(R, dtype=np.float64)
    trip = np.asarray(trip, dtype=np.int64)
    ga, gp, gb = triple_grads(model, E64[trip[:, 0]], R64[trip[:, 1]], E64[trip[:, 2]], np.asarray(g, dtype=np.float64), float(scale))
    dE, dR = np.zeros_like(E64), np.zeros_like(R64)
    np.add.at(dE, trip[:, 0], ga)
    np.add.at(dE, trip[:, 2], gb)
    np.add.at(dR, trip[:, 1], gp)
    absE, absR = np.zeros_like(E64), np.zeros_like(R64)      # sum of the terms' magnitudes: what a rounding bound scales with
    np.add.at(absE, trip[:, 0], np.abs(ga))
    np.add.at(absE, trip[:, 2], np.abs(gb))
    np.add.at(absR, trip[:, 1], np.abs(gp))
    return dE, dR, absE, absR
