"""Host statement of the batch-local Lp / N3 regulariser (include/emgraph_hip.h: emg_batchreg).  numpy only.

For the positives (s_i, p_i, o_i), i < B:   R = sum_i [ lam_ent (N(E[s_i]) + N(E[o_i])) + lam_rel N(R[p_i]) ]
  plain form    N(x) = sum_c |x_c|^p                          modulus form  N(x) = sum_j (x_j^2 + x_{j + k}^2)^(p / 2), k = k_int / 2
``rows_f32`` / ``batch_reg`` restate the device's gradient rows operation for operation in float32 (every numpy operation below is one
correctly rounded f32 operation, as the kernel's are) and its value (f32 terms, summed in double); ``value64`` / ``grad64`` are the
plain float64 form of R and of its gradient with respect to the two tables."""
import numpy as np

F = np.float32


def coefs(lam, p):
    """(coef_g, coef_v) = ((float)(lambda p), (float)lambda), rounded once from double"""
    return F(float(lam) * int(p)), F(float(lam))


def rows_f32(X, p, modulus, lam):
    """gradient rows [n, k_int] (float32) of the rows ``X`` and their f32 value terms ([n, k_int] plain, [n, k] modulus)"""
    X = np.ascontiguousarray(X, dtype=F)
    cg, _ = coefs(lam, p)
    zero, one = F(0), F(1)
    if not modulus:
        aw = np.abs(X)
        if p == 1:
            sg = np.where(X > zero, one, np.where(X < zero, -one, zero)).astype(F)
            return cg * sg, aw
        if p == 2:
            return cg * X, X * X
        return cg * (aw * X), (aw * aw) * aw
    k = X.shape[1] // 2
    assert X.shape[1] == 2 * k, "the modulus form needs an even k_int"
    a, b = X[:, :k], X[:, k:]
    s = a * a + b * b
    if p == 2:
        return np.concatenate([cg * a, cg * b], 1), s
    m = np.sqrt(s)
    assert m.dtype == F
    if p == 1:
        ms = np.where(m != zero, m, one)
        ga = np.where(m != zero, cg * (a / ms), zero).astype(F)
        gb = np.where(m != zero, cg * (b / ms), zero).astype(F)
        return np.concatenate([ga, gb], 1), m
    return np.concatenate([cg * (m * a), cg * (m * b)], 1), (m * m) * m


def row_values(terms):
    """per row: the f32 terms summed in double, ascending"""
    t = np.asarray(terms, dtype=np.float64)
    return np.cumsum(t, axis=1)[:, -1] if t.shape[1] else np.zeros(t.shape[0])


def batch_reg(E, R, pos, p, lam_ent, lam_rel, mod_ent, mod_rel):
    """what emg_batchreg writes for the positives ``pos`` [B, 3]: (contrib_ent [2 B, k_int], dest_ent [2 B], contrib_rel [B, k_int] or
    None, dest_rel [B] or None, value) — relation rows only if lam_rel != 0 in float32"""
    pos = np.asarray(pos, dtype=np.int64).reshape(-1, 3)
    ids_e = np.concatenate([pos[:, 0], pos[:, 2]])
    ge, te = rows_f32(np.asarray(E)[ids_e], p, mod_ent, lam_ent)
    value = float(np.sum(row_values(te) * float(coefs(lam_ent, p)[1])))
    cg_r, cv_r = coefs(lam_rel, p)
    if cg_r == 0 and cv_r == 0:
        return ge, ids_e.astype(np.int32), None, None, value
    gr, tr = rows_f32(np.asarray(R)[pos[:, 1]], p, mod_rel, lam_rel)
    value += float(np.sum(row_values(tr) * float(cv_r)))
    return ge, ids_e.astype(np.int32), gr, pos[:, 1].astype(np.int32), value


def _n64(X, p, modulus):
    X = np.asarray(X, dtype=np.float64)
    if not modulus:
        return (np.abs(X) ** p).sum(axis=1)
    k = X.shape[1] // 2
    return ((X[:, :k] ** 2 + X[:, k:] ** 2) ** (p / 2.0)).sum(axis=1)


def value64(E, R, pos, p, lam_ent, lam_rel, mod_ent, mod_rel):
    """R in float64"""
    pos = np.asarray(pos, dtype=np.int64).reshape(-1, 3)
    v = lam_ent * (_n64(np.asarray(E)[pos[:, 0]], p, mod_ent).sum() + _n64(np.asarray(E)[pos[:, 2]], p, mod_ent).sum())
    return float(v + lam_rel * _n64(np.asarray(R)[pos[:, 1]], p, mod_rel).sum())


def _dn64(X, p, modulus):
    X = np.asarray(X, dtype=np.float64)
    if not modulus:
        return p * np.abs(X) ** (p - 1) * np.sign(X)
    k = X.shape[1] // 2
    m2 = X[:, :k] ** 2 + X[:, k:] ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(m2 > 0, p * m2 ** (p / 2.0 - 1.0), 0.0)
    return np.concatenate([f * X[:, :k], f * X[:, k:]], 1)


def grad64(E, R, pos, p, lam_ent, lam_rel, mod_ent, mod_rel):
    """(dR/dE, dR/dR) in float64, every occurrence of a row counted"""
    pos = np.asarray(pos, dtype=np.int64).reshape(-1, 3)
    E, R = np.asarray(E, dtype=np.float64), np.asarray(R, dtype=np.float64)
    dE, dR = np.zeros_like(E), np.zeros_like(R)
    for col in (0, 2):
        np.add.at(dE, pos[:, col], lam_ent * _dn64(E[pos[:, col]], p, mod_ent))
    np.add.at(dR, pos[:, 1], lam_rel * _dn64(R[pos[:, 1]], p, mod_rel))
    return dE, dR


def scatter_rows(n_rows, rows, dest):
    """float64 [n_rows, k_int]: the gradient rows summed by destination"""
    out = np.zeros((n_rows, rows.shape[1]), dtype=np.float64)
    np.add.at(out, np.asarray(dest, dtype=np.int64), np.asarray(rows, dtype=np.float64))
    return out
