"""Host statement of shared negatives (include/emgraph_hip.h: emg_shared_forward / emg_shared_backward).  numpy only.

THE IDENTITY: a batch of B positives is cut into G = ceil(B / C) chunks of C consecutive rows; slot m = sd * eta + j has one draw per
chunk, ``chunk_codes[m * G + g]`` (replacement | keep_subject << 31), and the step is the ordinary step with
``codes[m * B + i] = chunk_codes[m * G + i // C]``.  ``dense_grads`` is a float64 restatement of the gradient of sum(g * score)
over the positives and the expanded negatives, scattered into dense tables."""
import numpy as np

TRANSE_L1, TRANSE_L2, DISTMULT, COMPLEX, HOLE, TRANSE_P, ROTATE = range(7)


def n_chunks(B, C):
    return -(-int(B) // int(C))


def expand_codes(chunk_codes, B, C, eta_total):
    """codes [eta_total * B] of the ordinary step from chunk_codes [eta_total * G]"""
    G = n_chunks(B, C)
    cc = np.asarray(chunk_codes).reshape(eta_total, G)
    out = np.empty((eta_total, B), dtype=cc.dtype)
    for m in range(eta_total):
        for i in range(B):
            out[m, i] = cc[m, i // C]
    return out.reshape(-1)


def split_codes(codes):
    """(replacement ids, keep_subject flags) of int32 codes"""
    c = np.asarray(codes).astype(np.int64) & 0xFFFFFFFF
    return (c & 0x7FFFFFFF).astype(np.int64), (c >> 31).astype(np.int64)


def negatives(pos, codes, eta_total):
    """[eta_total * B, 3] triples of the expanded codes (row m * B + i)"""
    pos = np.asarray(pos, dtype=np.int64)
    B = pos.shape[0]
    repl, keep = split_codes(codes)
    i = np.tile(np.arange(B), eta_total)
    s = np.where(keep == 1, pos[i, 0], repl)
    o = np.where(keep == 1, repl, pos[i, 2])
    return np.stack([s, pos[i, 1], o], 1)


def triple_grads(model, a, p, b, g, scale):
    """d(sum g * f)/d(a, p, b) for rows a, p, b [n, k_int] (float64) and upstream g [n]; f the model's score"""
    g = g[:, None]
    if model in (TRANSE_L1, TRANSE_L2, TRANSE_P):
        d = a + p - b
        if model == TRANSE_L1:
            u = np.sign(d)
        elif model == TRANSE_L2:
            u = d / np.sqrt((d * d).sum(1, keepdims=True))
        else:
            nrm = (np.abs(d) ** scale).sum(1, keepdims=True) ** (1.0 / scale)
            u = np.sign(d) * np.abs(d) ** (scale - 1.0) / nrm ** (scale - 1.0)
        return -g * u, -g * u, g * u
    if model == DISTMULT:
        return g * p * b, g * a * b, g * a * p
    n = a.shape[1] // 2
    ar, ai, br, bi = a[:, :n], a[:, n:], b[:, :n], b[:, n:]
    if model == ROTATE:
        cs, sn = np.cos(p[:, :n]), np.sin(p[:, :n])
        wr, wi = ar * cs - ai * sn, ar * sn + ai * cs
        dr, di = wr - br, wi - bi
        m = np.sqrt(dr * dr + di * di)
        ur, ui = dr / m, di / m
        ga = np.concatenate([-(ur * cs + ui * sn), -(ui * cs - ur * sn)], 1)
        gb = np.concatenate([ur, ui], 1)
        gp = np.concatenate([ur * wi - ui * wr, np.zeros_like(ur)], 1)
        return g * ga, g * gp, g * gb
    pr, pi = p[:, :n], p[:, n:]
    f = g * (scale if model == HOLE else 1.0)       # f = scale * Re<p, a, conj(b)>
    ga = np.concatenate([pr * br + pi * bi, pr * bi - pi * br], 1)
    gp = np.concatenate([ar * br + ai * bi, ar * bi - ai * br], 1)
    gb = np.concatenate([pr * ar - pi * ai, pr * ai + pi * ar], 1)
    return f * ga, f * gp, f * gb


def dense_grads(model, E, R, pos, codes, eta_total, g_pos, g_neg, scale):
    """(dE [n_ent, k_int], dR [n_rel, k_int]) in float64: the gradient rows of the positives (upstream g_pos [B]) and of the
    negatives of ``codes`` (g_neg [eta_total * B]) added up by destination"""
    E64, R64 = np.asarray(E, dtype=np.float64), np.asarray(R, dtype=np.float64)
    pos = np.asarray(pos, dtype=np.int64)
    trip = np.concatenate([pos, negatives(pos, codes, eta_total)], 0)
    g = np.concatenate([np.asarray(g_pos, dtype=np.float64), np.asarray(g_neg, dtype=np.float64)])
    ga, gp, gb = triple_grads(model, E64[trip[:, 0]], R64[trip[:, 1]], E64[trip[:, 2]], g, float(scale))
    dE, dR = np.zeros_like(E64), np.zeros_like(R64)
    np.add.at(dE, trip[:, 0], ga)
    np.add.at(dE, trip[:, 2], gb)
    np.add.at(dR, trip[:, 1], gp)
    return dE, dR


def scatter_rows(rows, dest, n_rows):
    """float64 sum of the gradient rows ``rows`` [n, k] by destination ``dest`` [n]"""
    out = np.zeros((n_rows, rows.shape[1]), dtype=np.float64)
    np.add.at(out, np.asarray(dest, dtype=np.int64), np.asarray(rows, dtype=np.float64))
    return out
