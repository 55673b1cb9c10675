"""Host references for SimplE (EMG_SIMPLE; include/emgraph_hip.h has the contract).  numpy and the committed C chain only, no device.

Rows are [h | t] (entities) and [r | r_inv] (relations), k columns per half; swap(x) exchanges the halves of a 2k-wide row and
    f(s, p, o) = scale * sum_{c < 2k} e_s[c] rel_p[c] swap(e_o)[c]        (scale = 1/2: the averaged form)

(a) score_f64 / score_two_sums_f64 / grads_f64 / queries_f64: float64 (tests/test_simple_host.py checks the gradients against
    central finite differences and the swap form against the two sums);
(b) queries_f32: the query rows as the device builds them — ONE float32 product per column;
(c) chain_f32: the canonical 1-vs-all chain on GIVEN query rows — oracle.c_oracle.scores_dense with HolE's id: the committed C chain,
    explicit fmaf ascending from +0, then the product with `scale`;
(d) cmp_int: the comparison integer int32(f32(score) * f32(1e5)) (EmbeddingModel.py:2010-2014); counts and ranks are assembled by the
    package's own host helpers (FilterIndex.csr, ranks_from_counts);
(e) the bounds of the comparisons with float64, each derived where it is defined, and the shared cases of tests/test_simple.py.
"""
import numpy as np

from oracle import c_oracle as co
from oracle import emgraph_oracle as orc

F32 = np.float32
MID = orc.MODEL_IDS
SCALE = 0.5
U = 2.0 ** -24          # unit roundoff of float32


def swap(x):
    """the two halves of the last axis exchanged"""
    k = x.shape[-1] // 2
    return np.concatenate([x[..., k:], x[..., :k]], -1)


def rows_f64(E, R, X):
    E = np.asarray(E, dtype=np.float64)
    R = np.asarray(R, dtype=np.float64)
    X = np.asarray(X)
    return E[X[:, 0]], R[X[:, 1]], E[X[:, 2]]


def score_f64(E, R, X, scale=SCALE):
    s, r, o = rows_f64(E, R, X)
    return scale * (s * r * swap(o)).sum(1)


def score_two_sums_f64(E, R, X):
    """1/2 (<h_s, r, t_o> + <h_o, r_inv, t_s>), the paper's statement"""
    s, r, o = rows_f64(E, R, X)
    k = s.shape[1] // 2
    return 0.5 * ((s[:, :k] * r[:, :k] * o[:, k:]).sum(1) + (o[:, :k] * r[:, k:] * s[:, k:]).sum(1))


def magnitude_f64(E, R, X, scale=SCALE):
    """scale * sum_c |e_s[c] rel[c] swap(e_o)[c]|: what the score's error bound is relative to"""
    return score_f64(np.abs(E), np.abs(R), X, scale)


def grads_f64(E, R, X, g, scale=SCALE):
    """(dE [n_ent, 2k], dR [n_rel, 2k]) of sum_t g_t f(X_t), float64, np.add.at (a triple with s == o adds both entity rows to one row):
    df/de_s = scale rel o swap(e_o), df/de_o = scale swap(rel o e_s), df/drel = scale e_s o swap(e_o)"""
    s, r, o = rows_f64(E, R, X)
    w = scale * np.asarray(g, dtype=np.float64)[:, None]
    dE = np.zeros(np.asarray(E).shape, np.float64)
    dR = np.zeros(np.asarray(R).shape, np.float64)
    X = np.asarray(X)
    np.add.at(dE, X[:, 0], w * r * swap(o))
    np.add.at(dE, X[:, 2], w * swap(r * s))
    np.add.at(dR, X[:, 1], w * s * swap(o))
    return dE, dR


def grad_terms_f64(E, R, X, g, scale=SCALE):
    """sum of |terms| feeding every element of (dE, dR): the gradients of the absolute values"""
    return grads_f64(np.abs(E), np.abs(R), X, np.abs(g), scale)


def queries_f64(E, R, X, obj):
    """float64 query rows [n, 2k]: object side (s kept, scored against e_o) q = swap(rel) o swap(e_s); subject side (o kept, scored
    against e_s) q = rel o swap(e_o)"""
    s, r, o = rows_f64(E, R, X)
    return swap(r) * swap(s) if obj else r * swap(o)


def queries_f32(E, R, X, obj):
    """the same rows in float32: one correctly rounded product per column (numpy float32 `*`)"""
    E = np.asarray(E, dtype=F32)
    R = np.asarray(R, dtype=F32)
    X = np.asarray(X)
    s, r, o = E[X[:, 0]], R[X[:, 1]], E[X[:, 2]]
    q = swap(r) * swap(s) if obj else r * swap(o)
    assert q.dtype == F32
    return q


def chain_f32(Q, E, scale=SCALE):
    """the canonical chain of every (query row, entity row) pair, float32 [n_rows, n_ent]: acc = fmaf(q_c, e_c, acc), c ascending from
    +0, then acc * scale — the committed C chain under HolE's id (oracle/emg_oracle.c)"""
    Q = np.ascontiguousarray(Q, dtype=F32)
    E = np.ascontiguousarray(E, dtype=F32)
    assert Q.shape[1] == E.shape[1] and Q.shape[1] % 2 == 0
    return co.scores_dense(MID["HolE"], Q, E, Q.shape[1], float(scale))


def cmp_int(phi):
    """int32(f32(phi) * f32(1e5)) in float32 arithmetic (scores far inside the int32 range)"""
    return (np.asarray(phi).astype(F32) * F32(100000.0)).astype(np.int32)


def score_bound(E, R, X, scale=SCALE):
    """|f32 - f64| <= (2k + 3) 2^-24 scale sum_c |e_s[c] rel[c] swap(e_o)[c]|: the standard bound of a 2k-term sum in any order
    (gamma_{2k - 1}), the two roundings of each triple product (the product e_s rel, the fused multiply-add's own), the product with
    scale — 2k + 2 roundings on any path from a term to the result, first order, one more for the higher-order terms"""
    k_int = np.asarray(E).shape[1]
    return (k_int + 3) * U * magnitude_f64(E, R, X, scale)


def grad_bound(E, R, X, g, eta, scale=SCALE):
    """per element of (dE, dR): (eta + 4) 2^-24 sum |terms feeding that element| — a term g scale (x y) carries three roundings (g
    scale, x y, their product), a slot adds at most 1 + eta terms in sequence (eta roundings), one more for the higher-order terms; the
    slots of one destination are added in float64 by the test"""
    tE, tR = grad_terms_f64(E, R, X, g, scale)
    return (eta + 4) * U * tE, (eta + 4) * U * tR


def topn_host(S, ids, top_n, excluded=None):
    """(ids [n_rows, top_n], scores) of a host sort of the scores S [n_rows, n_cand] of the candidates ``ids`` in the contract's order:
    higher score first, -0 == +0, ties by ascending entity id; ``excluded[r]``: ids row r leaves out; short rows (-1, -inf)"""
    n_rows = S.shape[0]
    out_i = np.full((n_rows, top_n), -1, np.int32)
    out_s = np.full((n_rows, top_n), -np.inf, F32)
    ids = np.asarray(ids)
    for r in range(n_rows):
        keep = np.ones(len(ids), bool) if excluded is None else ~np.isin(ids, excluded[r])
        s, i = S[r, keep] + F32(0.0), ids[keep]
        order = np.lexsort((i, -s.astype(np.float64)))[:top_n]
        out_i[r, :len(order)], out_s[r, :len(order)] = i[order], s[order]
    return out_i, out_s


# ---- the shared cases of tests/test_simple.py ------------------------------------------------------------------------------------
N_ENT, N_REL, N_POS = 300, 6, 130      # 130 positives / query rows: past the 64- and 128-row tile edges; 300 entities: past two 128-tiles


def training_case(k, eta):
    """(E, R, X, codes, xneg, keep_s, repl): tables uniform in +-0.5; X[0] has s == o; the first negative of X[1] replaces the object by
    the kept subject, the first negative of X[2] the subject by the kept object.  codes: eta-major replacement | keep_subject << 31,
    xneg the corruptions they stand for."""
    rs = np.random.RandomState(1000 * k + eta)
    E = rs.uniform(-0.5, 0.5, (N_ENT, 2 * k)).astype(F32)
    R = rs.uniform(-0.5, 0.5, (N_REL, 2 * k)).astype(F32)
    X = np.stack([rs.randint(0, N_ENT, N_POS), rs.randint(0, N_REL, N_POS), rs.randint(0, N_ENT, N_POS)], 1).astype(np.int32)
    X[0, 2] = X[0, 0]
    repl = rs.randint(0, N_ENT, eta * N_POS).astype(np.int64)
    keep_s = rs.randint(0, 2, eta * N_POS).astype(np.int64)
    keep_s[1], repl[1] = 1, X[1, 0]        # (negative j of positive g is entry j * N_POS + g)
    keep_s[2], repl[2] = 0, X[2, 2]
    codes = (repl | (keep_s << 31)).astype(np.uint32).view(np.int32)
    pos = np.tile(X, (eta, 1))
    xneg = pos.copy()
    xneg[:, 2] = np.where(keep_s == 1, repl, pos[:, 2])
    xneg[:, 0] = np.where(keep_s == 1, pos[:, 0], repl)
    return E, R, X, codes, xneg.astype(np.int32), keep_s.astype(np.int32), repl.astype(np.int32)
