"""Host references for RotatE (EMG_ROTATE; include/emgraph_hip.h has the contract).  numpy only.

(a) score_f64 / grads_f64: the score f = -sum_j |s_j r_j - o_j|, r_j = exp(i theta_j), and its analytic gradients in float64
    (tests/test_rotate_host.py checks them against central finite differences);
(b) chain_f32: the canonical 1-vs-all chain restated in float32 from GIVEN query rows — numpy float32 `-`, `*`, `+`, `sqrt`, each
    one correctly rounded IEEE operation, in the kernel's order: the device's bits;
(c) cmp_int: the comparison integer int32(f32(score) * f32(1e5)) (EmbeddingModel.py:2010-2014), as tests/test_link_ranking.py
    takes it on the host; counts and ranks are assembled by the package's own host helpers (FilterIndex.csr, ranks_from_counts).
"""
import numpy as np

F32 = np.float32


def split(E, R, X):
    """float64 (s_re, s_im, theta, o_re, o_im) of the triples X; rows are [re(k) | im(k)], phases in the first k relation columns"""
    E = np.asarray(E, dtype=np.float64)
    R = np.asarray(R, dtype=np.float64)
    k = E.shape[1] // 2
    s, o = E[X[:, 0]], E[X[:, 2]]
    return s[:, :k], s[:, k:], R[X[:, 1], :k], o[:, :k], o[:, k:]


def moduli_f64(E, R, X):
    """|s_j r_j - o_j| per (triple, coordinate), float64 [n, k]"""
    sr, si, th, orr, oi = split(E, R, X)
    c, sn = np.cos(th), np.sin(th)
    return np.hypot(sr * c - si * sn - orr, sr * sn + si * c - oi)


def score_f64(E, R, X):
    return -moduli_f64(E, R, X).sum(1)


def grads_f64(E, R, X, g):
    """(dE [n_ent, 2k], dR [n_rel, 2k]) of sum_t g_t f(X_t), float64: with w = s r, d = w - o, u = d / |d| (0 where |d| = 0)
    df/ds = -u conj(r), df/do = +u, df/dtheta = u_re w_im - u_im w_re; relation columns [k, 2k) stay 0"""
    sr, si, th, orr, oi = split(E, R, X)
    k = sr.shape[1]
    c, sn = np.cos(th), np.sin(th)
    wr, wi = sr * c - si * sn, sr * sn + si * c
    dr, di = wr - orr, wi - oi
    m = np.hypot(dr, di)
    safe = np.where(m > 0, m, 1.0)
    ur, ui = np.where(m > 0, dr / safe, 0.0), np.where(m > 0, di / safe, 0.0)
    g = np.asarray(g, dtype=np.float64)[:, None]
    dE = np.zeros((np.asarray(E).shape[0], 2 * k))
    dR = np.zeros((np.asarray(R).shape[0], 2 * k))
    np.add.at(dE, X[:, 0], g * np.concatenate([-(ur * c + ui * sn), -(ui * c - ur * sn)], 1))
    np.add.at(dE, X[:, 2], g * np.concatenate([ur, ui], 1))
    np.add.at(dR, X[:, 1], g * np.concatenate([ur * wi - ui * wr, np.zeros_like(ur)], 1))
    return dE, dR


def queries_f64(E, R, T, obj_side):
    """float64 query rows [n, 2k]: object side q = s r, subject side q = o conj(r)"""
    sr, si, th, orr, oi = split(E, R, T)
    c, sn = np.cos(th), np.sin(th)
    if obj_side:
        return np.concatenate([sr * c - si * sn, sr * sn + si * c], 1)
    return np.concatenate([orr * c + oi * sn, oi * c - orr * sn], 1)


def chain_f32(Q, E):
    """the canonical chain, float32 [n_rows, n_cand]: j ascending from acc = +0, dr = q_re[j] - e_re[j], di = q_im[j] - e_im[j],
    m = sqrt(dr * dr + di * di) (two products, their sum, the root: four roundings), acc = acc + m; the score is -acc"""
    Q = np.ascontiguousarray(Q, dtype=F32)
    E = np.ascontiguousarray(E, dtype=F32)
    k = Q.shape[1] // 2
    assert Q.shape[1] == 2 * k == E.shape[1]
    acc = np.zeros((Q.shape[0], E.shape[0]), dtype=F32)
    for j in range(k):
        dr = Q[:, j, None] - E[None, :, j]
        di = Q[:, k + j, None] - E[None, :, k + j]
        acc = acc + np.sqrt(dr * dr + di * di)
        assert acc.dtype == F32
    return -acc


def cmp_int(phi):
    """int32(f32(phi) * f32(1e5)) in float32 arithmetic (scores far inside the int32 range)"""
    return (np.asarray(phi).astype(F32) * F32(100000.0)).astype(np.int32)


def topn_host(S, ids, top_n, excluded=None):
    """(ids [n_rows, top_n], scores) of a host sort of the scores S [n_rows, n_cand] of the candidates ``ids``: higher score first,
    ties by ascending entity id; ``excluded[r]``: entity ids row r leaves out; short rows padded with (-1, -inf)"""
    n_rows = S.shape[0]
    out_i = np.full((n_rows, top_n), -1, np.int32)
    out_s = np.full((n_rows, top_n), -np.inf, F32)
    ids = np.asarray(ids)
    for r in range(n_rows):
        keep = np.ones(len(ids), bool) if excluded is None else ~np.isin(ids, excluded[r])
        s, i = S[r, keep] + F32(0.0), ids[keep]          # (+0: -0 and +0 are one score)
        order = np.lexsort((i, -s.astype(np.float64)))[:top_n]
        out_i[r, :len(order)], out_s[r, :len(order)] = i[order], s[order]
    return out_i, out_s


# ---- the shared case of tests/test_rotate.py (numpy only: its conditioning is checked without a device) ---------------------------
N_ENT, N_REL, N_POS = 130, 5, 70          # two candidate tiles of 64 and a tail; a second block of 64 rows / positives with a tail
PLANT = 129                               # the entity of the planted triple (PLANT, 4, PLANT): nobody else reads or writes its row
MIN_MODULUS = 1e-3


def training_case(k, eta, phase=np.pi):
    """(E, R, X, codes, xneg): entity rows uniform in +-0.5, phases uniform in +-``phase`` (relation columns [k, 2k) zero), relation 4
    all zero and used by X[0] = (PLANT, 4, PLANT) alone — d = 0 exactly in every coordinate; every other triple and every
    replacement stays below entity 128.  codes: eta-major replacement | keep_subject << 31, xneg the corruptions they stand for."""
    rs = np.random.RandomState(1000 * k + 10 * eta + int(phase))
    E = rs.uniform(-0.5, 0.5, (N_ENT, 2 * k)).astype(F32)
    R = np.zeros((N_REL, 2 * k), F32)
    R[:, :k] = rs.uniform(-phase, phase, (N_REL, k))
    R[4] = 0.0
    X = np.stack([rs.randint(0, 128, N_POS), rs.randint(0, 4, N_POS), rs.randint(0, 128, N_POS)], 1).astype(np.int32)
    X[0] = (PLANT, 4, PLANT)
    repl = rs.randint(0, 128, eta * N_POS).astype(np.int64)
    keep_s = rs.randint(0, 2, eta * N_POS).astype(np.int64)
    codes = (repl | (keep_s << 31)).astype(np.uint32).view(np.int32)
    pos = np.tile(X, (eta, 1))
    xneg = pos.copy()
    xneg[:, 2] = np.where(keep_s == 1, repl, pos[:, 2])
    xneg[:, 0] = np.where(keep_s == 1, pos[:, 0], repl)
    return E, R, X, codes, xneg.astype(np.int32), keep_s.astype(np.int32), repl.astype(np.int32)


def well_conditioned(E, R, X, xneg):
    """the condition of the gradient comparison: every modulus of every scored triple but the planted one is >= MIN_MODULUS, so u = d / m
    is well conditioned in float32"""
    return min(moduli_f64(E, R, X[1:]).min(), moduli_f64(E, R, xneg).min()) >= MIN_MODULUS
