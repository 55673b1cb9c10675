"""The tables and shapes of the k-means tests (tests/test_kmeans_host.py chooses and checks them on the CPU,
tests/test_kmeans.py runs them on the GPU)."""
import numpy as np

from tests import _chain_ref as cr

F32 = np.float32

# (n, k, C): every n of {1, 2, 63, 64, 65, 130, 257, 1000} (the 64-row A tile, several workgroups, the 256-row blocks of the
# counting sort), every k of {1, 3, 31, 32, 33, 40, 100} (the k-tile tail), every C <= n of {1, 2, 6, 63, 64, 65, 130} (the 64-wide
# B tile: the minimum is carried across tiles)
SHAPES = [(1, 1, 1), (2, 3, 2), (2, 32, 1), (63, 31, 6), (63, 40, 63), (64, 32, 64), (64, 3, 2), (65, 33, 65), (65, 100, 6),
          (130, 40, 130), (130, 31, 64), (130, 1, 2), (257, 32, 65), (257, 100, 6), (257, 33, 63), (1000, 40, 6), (1000, 3, 130),
          (1000, 31, 64), (1000, 100, 2), (1000, 1, 6)]
MAX_ITER = 60


def integers(n, k, seed=0):
    """small integers in [-3, 3]: every distance tie is exact (a row is often equally near two centres: the lower index must
    win) and at k <= 3 many rows coincide, so clusters go empty"""
    rng = np.random.default_rng([seed, n, k, 9])
    return rng.integers(-3, 4, size=(n, k)).astype(F32)


def tables(n, k):
    """name -> table: the integer table and _chain_ref's real-valued makers (which plant identical rows)"""
    out = {"integers": integers(n, k)}
    for name, maker in cr.MAKERS.items():
        out[name] = maker(n, k)
    return out


def start_rows(n, C, seed=0):
    """C different rows of the table as the initial centres (planted identical rows can give two equal centres)"""
    return np.random.default_rng([seed, n, C, 11]).choice(n, C, replace=False)


# ---- separated tables: the ones scikit-learn is compared on ------------------------------------------------
SEPARATION = 0.05   # every assignment margin (second - best) / second of a separated table's run exceeds this


def separated(n, k, C, seed=0):
    """C centres on the lattice 4 Z^k, all different, and n rows centre + U(-0.5, 0.5)^k with every cluster populated: a row is
    at most 0.5 sqrt(k) from its own centre and at least 4 - 0.5 sqrt(k) from another.  Stated separation: with the start
    below every assignment margin of the run is above SEPARATION (tests/test_kmeans_host.py asserts it)."""
    rng = np.random.default_rng([seed, n, k, C, 12])
    assert n >= C
    seen, centres = set(), []
    while len(centres) < C:
        c = tuple(rng.integers(-3, 4, size=k).tolist())
        if c not in seen:
            seen.add(c)
            centres.append(c)
    centres = 4.0 * np.asarray(centres, np.float64)
    owner = np.concatenate([np.arange(C), rng.integers(0, C, size=n - C)])
    rng.shuffle(owner)
    X = centres[owner] + rng.uniform(-0.5, 0.5, size=(n, k))
    first = np.array([np.nonzero(owner == c)[0][0] for c in range(C)])   # one row of every cluster: the start
    return X.astype(F32), first


SEPARATED = [(130, 8, 6), (257, 12, 6), (1000, 8, 65), (300, 16, 2)]


# ---- cluster sizes around the update's chunk length -----------------------------------------------------------
def sized_clusters(sizes, k=24, seed=0):
    """(table, start centres, owner): real-valued clusters of exactly the given sizes around far-apart centres, the rows in a
    shuffled order, so that a cluster's members lie in many 256-row blocks of the sort; from the true centres as the start
    the first assignment is ``owner``"""
    rng = np.random.default_rng([seed, len(sizes), k, 13])
    centres = np.zeros((len(sizes), k))
    centres[np.arange(len(sizes)), np.arange(len(sizes)) % k] = 10.0 * (1 + np.arange(len(sizes)) // k)
    owner = np.repeat(np.arange(len(sizes)), sizes)
    rng.shuffle(owner)
    X = centres[owner] + rng.standard_normal((len(owner), k)) * 0.3
    return X.astype(F32), centres.astype(F32), owner.astype(np.int32)


SIZED = {"around_the_chunk": [255, 256, 257, 1, 231], "one_holds_most": [900, 50, 50]}

# ---- the tol > 0 stop -----------------------------------------------------------------------------------------
TOL_CASE = dict(maker="normal", n=1000, k=40, C=6, seed=5, tol=1e-2)   # stops on the shift after 16 updates


def tol_case():
    X = cr.MAKERS[TOL_CASE["maker"]](TOL_CASE["n"], TOL_CASE["k"])
    start = X[np.random.default_rng(TOL_CASE["seed"]).choice(TOL_CASE["n"], TOL_CASE["C"], replace=False)]
    return X, start, TOL_CASE["tol"]


# ---- seeding --------------------------------------------------------------------------------------------------
SEED_CASES = [("blobs", 257, 33, 6, 0), ("blobs", 1000, 40, 65, 1), ("normal", 130, 31, 130, 2), ("mixed", 1000, 100, 6, 3),
              ("integers", 1000, 3, 64, 4), ("normal", 65, 1, 2, 5), ("integers", 2, 3, 2, 6)]
