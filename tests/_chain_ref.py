"""The distances of the discovery contract, on the host (no device): the expected result of emg_rows_within, emg_rows_dbscan
and the public discovery functions on REAL-VALUED tables, to the bit.

The contract defines l2 as sqrtf of the k-ordered f32 chain fmaf(d, d, acc), d = a_k - b_k, and cosine as
1 - the k-ordered chain fmaf(a_k, b_k, acc) on normalised rows.  oracle/emg_oracle.c::orc_chain_score is that chain in C
(explicit fmaf, -ffp-contract=off); everything here is built on oracle.c_oracle.scores_dense.  On tables of small integers
any arithmetic gives these bits; on the tables made below a chain in another order, a Gram form, an unfused product or a
k-tile tail with one step too many does not (tests/test_chain_ref_host.py measures it)."""
import numpy as np

from oracle import c_oracle as co
from oracle import emgraph_oracle as orc

F32 = np.float32
MID = orc.MODEL_IDS


def _rows(a):
    a = np.ascontiguousarray(a, dtype=F32)
    assert a.ndim == 2
    return a


def l2_chain(A, B):
    """f32 [n_a, n_b]: sqrtf of the chain fmaf(d, d, acc), d = a_k - b_k, k ascending (a zero distance is +0)"""
    A, B = _rows(A), _rows(B)
    assert A.shape[1] == B.shape[1]
    return -co.scores_dense(MID["TransE_L2"], A, B, A.shape[1], 1.0)


def cosine_chain(NA, NB):
    """f32 [n_a, n_b]: 1 - the chain fmaf(a_k, b_k, acc), k ascending, the subtraction rounded once in f32.  NA, NB are the
    rows the device's rows_normalize produced, copied back: the chain is pinned on exactly those operands."""
    NA, NB = _rows(NA), _rows(NB)
    assert NA.shape[1] == NB.shape[1]
    dot = co.scores_dense(MID["DistMult"], NA, NB, NA.shape[1], 1.0)
    out = F32(1) - dot
    assert out.dtype == F32
    return out


def others(n_a, n_b, self_offset):
    """bool [n_a, n_b]: False where column j IS row i (A = rows [self_offset, self_offset + n_a) of B; -1: foreign rows)"""
    other = np.ones((n_a, n_b), bool)
    if self_offset >= 0:
        other[np.arange(n_a), self_offset + np.arange(n_a)] = False
    return other


def brute(dist, self_offset, radius):
    """(count int32, nn_dist f32, nn_id int32, sorted packed pairs int64): the contract of emg_rows_within from a distance
    matrix.  count: the other rows with d <= radius (a NaN is within nothing).  Nearest: the minimum of (distance, id) over
    the other rows whose distance is no NaN — +inf is a distance like any other — and (inf, -1) if there is none."""
    dist = np.asarray(dist, dtype=F32)
    n_a, n_b = dist.shape
    other = others(n_a, n_b, self_offset)
    with np.errstate(invalid="ignore"):
        within = other & (dist <= F32(radius))
    valid = other & ~np.isnan(dist)
    nn_dist = np.full(n_a, np.inf, F32)
    nn_id = np.full(n_a, -1, np.int32)
    for r in range(n_a):
        cand = np.nonzero(valid[r])[0]
        if cand.size:
            d = dist[r, cand]
            j = cand[d == d.min()][0]          # cand ascends: the lowest id among the minima
            nn_dist[r], nn_id[r] = dist[r, j], j
    i, j = np.nonzero(within)
    return within.sum(1).astype(np.int32), nn_dist, nn_id, np.sort((i.astype(np.int64) << 32) | j)


def neighbours(dist, cand, n):
    """(ids int32 [n_q, n], distances f32 [n_q, n]) in (distance, id) order, padded with -1 / +inf: column c of ``dist`` is
    candidate ``cand[c]``"""
    dist, cand = np.asarray(dist, dtype=F32), np.asarray(cand)
    ids = np.full((dist.shape[0], n), -1, np.int32)
    out = np.full((dist.shape[0], n), np.inf, F32)
    for r in range(dist.shape[0]):
        order = np.lexsort((cand, dist[r]))[:n]
        ids[r, :len(order)] = cand[order]
        out[r, :len(order)] = dist[r][order]
    return ids, out


def core_eps(dist, i, m):
    """the eps at which row i is core for min_samples = m ONLY through a pair lying exactly at eps: the (m - 1)-th smallest
    distance from row i to another row (with the row's own 0 that is the m-th smallest entry of row i of the l2 matrix)"""
    row = np.delete(np.asarray(dist[i], dtype=F32), i)
    row = np.sort(row[~np.isnan(row)])
    return float(row[m - 2])


def within_matrix(dist, eps):
    """the boolean matrix tests/_dbscan_ref.py takes: d <= eps (NaN: no), every row within eps of itself"""
    with np.errstate(invalid="ignore"):
        return (np.asarray(dist, dtype=F32) <= F32(eps)) | np.eye(len(dist), dtype=bool)


# ---- tables -------------------------------------------------------------------------------------------
def plant(X):
    """Plants, when n allows: bit-identical copies (the last row is row 0; rows 40 and 62 are row 7; at n >= 65 row 64, the
    first of the second 64-row tile, is row 1); a row that is np.nextafter of another in every coordinate (row 5 of row 3);
    and a row equal to another in all but the LAST coordinate (row 9 of row 8): that pair differs only in the last chain
    step, which at k % 32 != 0 lies in the k-tile tail."""
    n, k = X.shape
    if n >= 63:
        X[40] = X[7]
        X[62] = X[7]
        X[5] = np.nextafter(X[3], F32(np.inf))
        X[9] = X[8]
        X[9, k - 1] = X[8, k - 1] + F32(0.5) * np.abs(X[8]).max()
    if n >= 65:
        X[64] = X[1]
    if n >= 2:
        X[n - 1] = X[0]
    return X


def normal(n, k, scale=0.1, seed=0):
    """normal entries of the given scale"""
    rng = np.random.default_rng([seed, n, k, 1])
    return plant((rng.standard_normal((n, k)) * scale).astype(F32))


def blobs(n, k, seed=0):
    """6 centres N(0, 0.3^2), points centre + N(0, 0.02^2), a tenth of the rows replaced by N(0, 0.3^2) noise"""
    rng = np.random.default_rng([seed, n, k, 2])
    centres = rng.standard_normal((6, k)) * 0.3
    X = centres[rng.integers(0, 6, size=n)] + rng.standard_normal((n, k)) * 0.02
    noise = rng.random(n) < 0.1
    X[noise] = rng.standard_normal((int(noise.sum()), k)) * 0.3
    return plant(X.astype(F32))


def mixed(n, k, seed=0):
    """normal 0.1 with every seventh column multiplied by 1000: the large columns dominate and the small ones sit near the
    rounding of the running sum"""
    rng = np.random.default_rng([seed, n, k, 3])
    X = rng.standard_normal((n, k)) * 0.1
    X[:, ::7] *= 1000.0
    return plant(X.astype(F32))


MAKERS = {"normal": normal, "blobs": blobs, "mixed": mixed}


def float64_l2(A, B):
    """the correctly rounded distance: differences, squares and sum in float64, one rounding to f32 at the end"""
    A64, B64 = np.asarray(A, np.float64), np.asarray(B, np.float64)
    out = np.empty((len(A64), len(B64)), F32)
    for r in range(len(A64)):
        d = A64[r][None, :] - B64
        out[r] = np.sqrt((d * d).sum(1))
    return out
