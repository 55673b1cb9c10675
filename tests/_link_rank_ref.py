"""Pin on the reference's semantics of ranking through a score link (EmbeddingModel.py:1868-1879, then perform_comparision
:2010-2033): the link is applied to the positive's score and to every corruption's score, and int32(phi(score) * 1e5) is compared.

The device forms phi with float32 libm calls whose error is not known here, so this restatement cannot name ONE rank per row.
It takes the link in float64 and turns every value's comparison integer into an INTERVAL: the device's float32 phi is assumed
within 8 float32 ulp of the float64 value (an assumption: libm's error on the device is not measured here), and the float32
product with 1e5 adds half an ulp of the product.  Counting the candidates that reach the positive for certain / possibly gives
[rank_lo, rank_hi] per (triple, side) row of the unfiltered or filtered 'worst' rank; the GPU test asserts the device's ranks lie
inside, the host test that most rows are TIGHT (rank_lo == rank_hi) so that the pin is not vacuous.

Raw scores: the tables of tests/golden/ranks.npz are multiples of 1/4 at k = 4, so every product and partial sum of the chains is
exact in float32 — the float64 value computed here IS the device's raw score, and equal raw scores are equal bits: certain ties.

Softplus (custom_softplus, log(1 + 9999 e^x)) is left out: its values reach 1e6 quanta, where one float32 ulp is a tenth of a cell
and only 0-14 of 40 rows are tight; it is covered by the device-bits tests of tests/test_link_ranking.py alone."""
import numpy as np

LINKS = ("tanh", "sigmoid")
ULPS = 8.0


def raw_scores(name, E, R, T, obj_side):
    """float64 raw scores [len(T), n_ent] of every corruption of one side (the positive sits at its own entity's column)"""
    E, R = E.astype(np.float64), R.astype(np.float64)
    s, p, o = E[T[:, 0]], R[T[:, 1]], E[T[:, 2]]
    n = E.shape[1] // 2
    if name == "TransE":        # L1, as the golden's tables were ranked
        q = s + p if obj_side else o - p
        return -np.abs(q[:, None, :] - E[None, :, :]).sum(-1)
    if name == "DistMult":
        q = p * (s if obj_side else o)
        return q @ E.T
    pr, pi = p[:, :n], p[:, n:]
    x = s if obj_side else o
    xr, xi = x[:, :n], x[:, n:]
    if obj_side:                # <[p_r s_r - p_i s_i | p_r s_i + p_i s_r], [e_r | e_i]>
        q = np.concatenate([pr * xr - pi * xi, pr * xi + pi * xr], 1)
    else:                       # <[p_r o_r + p_i o_i | p_r o_i - p_i o_r], [e_r | e_i]>
        q = np.concatenate([pr * xr + pi * xi, pr * xi - pi * xr], 1)
    sc = q @ E.T
    return sc * (2.0 / n) if name == "HolE" else sc


def phi64(link, x):
    if link == "tanh":
        return np.tanh(x)
    if link == "sigmoid":
        return 1.0 / (1.0 + np.exp(-x))
    raise ValueError(link)


def cmp_interval(link, x):
    """[lo, hi] of int32(float32(phi(x)) * float32(1e5)) under the 8-ulp assumption (module docstring)"""
    ph = phi64(link, x)
    v = ph * 1e5
    err = ULPS * np.spacing(np.abs(ph).astype(np.float32)).astype(np.float64) * 1e5 + 0.5 * np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)
    return np.trunc(v - err).astype(np.int64), np.trunc(v + err).astype(np.int64)


def rank_intervals(name, link, E, R, T, obj_ptr=None, obj_idx=None, sub_ptr=None, sub_idx=None):
    """(rank_lo, rank_hi) int64 [len(T), 2] = [subject side, object side] of the 'worst' rank: 1 + #{candidates whose integer
    reaches the positive's}, the candidates of a row's filter list (which holds the positive's own entity) not counted when the
    lists are given — the assembly of EmbeddingModel.py:1966-1986."""
    T = np.asarray(T, np.int64)
    out_lo, out_hi = np.zeros((len(T), 2), np.int64), np.zeros((len(T), 2), np.int64)
    for col, obj_side in ((1, True), (0, False)):
        raw = raw_scores(name, E, R, T, obj_side)
        tgt = T[:, 2] if obj_side else T[:, 0]
        lo, hi = cmp_interval(link, raw)
        ptr, idx = (obj_ptr, obj_idx) if obj_side else (sub_ptr, sub_idx)
        for i in range(len(T)):
            same = raw[i] == raw[i, tgt[i]]                      # equal raw scores are equal bits on the device: ties for certain
            sure = same | (lo[i] >= hi[i, tgt[i]])
            maybe = same | (hi[i] >= lo[i, tgt[i]])
            if ptr is not None:
                drop = np.zeros(raw.shape[1], bool)
                drop[idx[ptr[i]:ptr[i + 1]]] = True
                sure, maybe = sure & ~drop, maybe & ~drop
            out_lo[i, col], out_hi[i, col] = 1 + sure.sum(), 1 + maybe.sum()
    return out_lo, out_hi
