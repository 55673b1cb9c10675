"""The tables and parameter sets of tests/test_clusters.py (no device): shared with tests/test_clusters_host.py, which checks
on the CPU that the reference gives each of them the structure the GPU test relies on.

All l2 tables hold small integers: every squared distance is an integer that f32 holds exactly whatever the summation order,
and sqrtf of it is correctly rounded — the brute force below is the expected distance to the bit, ties at the radius included."""
import numpy as np

F32 = np.float32
N_RANDOM = (1, 2, 63, 64, 65, 257, 1000)
K_RANDOM = (1, 3, 37, 100)
MIN_SAMPLES = (1, 2, 3, 5)


def distances_l2(A):
    """(f32 distances of the self-join, integer squared distances): small integers, so float64 products and sums are exact"""
    A64 = A.astype(np.float64)
    sq = (A64 * A64).sum(1)
    d2 = sq[:, None] + sq[None, :] - 2 * (A64 @ A64.T)
    assert (d2 == np.rint(d2)).all() and d2.max(initial=0) < 2 ** 24
    return np.sqrt(d2.astype(F32)), d2          # exact integers below 2^24: the f32 square root is correctly rounded


def within_l2(A, eps):
    return distances_l2(A)[0] <= F32(eps)


def int_table(rng, n, k):
    """integers in [-3, 3]; a few rows are bit-identical copies of others (cores at eps = 0)"""
    B = rng.integers(-3, 4, size=(n, k)).astype(F32)
    if n >= 2:
        B[n - 1] = B[0]
    if n >= 63:
        B[40] = B[7]
        B[62] = B[7]
        B[5] = B[0]
        B[33] = B[7]
        B[34] = B[7]
    return B


def random_cases(n):
    """[(table, k, [(m, eps)])]: for every k the radii 0, sqrtf(m) for a squared distance m that occurs (pairs AT the radius
    count) and one above the maximum; m is the integer the radius stands for (None above the maximum: m = max)"""
    rng = np.random.default_rng(4000 + n)
    out = []
    for k in K_RANDOM:
        B = int_table(rng, n, k)
        d2 = distances_l2(B)[1]
        off = np.sort(d2[~np.eye(n, dtype=bool)])
        radii = [(0, 0.0)]
        if off.size:
            m = int(off[off.size // 40])
            radii.append((m, float(np.sqrt(F32(m)))))
            radii.append((int(off[-1]) + 1, float(np.sqrt(F32(off[-1]))) + 1.0))
        else:
            radii.append((1, 1.0))
        out.append((B, k, radii))
    return out


def _pad(points, k):
    P = np.zeros((len(points), k), F32)
    pts = np.asarray(points, F32)
    P[:, :pts.shape[1]] = pts
    return P


def blobs():
    """three 10 x 10 unit grids far apart, their rows interleaved (a cluster spans every A workgroup and B tile of the 309
    rows), and nine isolated points.  eps = 1, min_samples = 5: the 64 interior points of a grid are core (4 neighbours and
    themselves), its 32 edge points are border rows (3 neighbours, one of them interior), its 4 corners are noise (their 2
    neighbours are edge points: not core)."""
    grids = []
    for ox, oy in ((0, 0), (100, 0), (0, 100)):
        g = np.stack(np.meshgrid(np.arange(10), np.arange(10), indexing="ij"), -1).reshape(-1, 2)
        grids.append(g + np.array([ox, oy]))
    inter = np.stack(grids, 1).reshape(-1, 2)                  # grid 0 row 0, grid 1 row 0, grid 2 row 0, grid 0 row 1, ...
    lone = np.array([[50 + 7 * t, 50 + 5 * t] for t in range(9)])
    pts = np.concatenate([inter[:150], lone[:4], inter[150:], lone[4:]])
    return _pad(pts, 3)


def chain():
    """1000 points one unit apart in REVERSED index order (row r sits at 999 - r), then a second chain of 400 far away (rows in
    ascending order) and one isolated point.  eps = 1, min_samples = 2: every chain point is core; the union hooks under non-roots and climbs."""
    x = np.concatenate([np.arange(999, -1, -1), 1200 + np.arange(400), [1800]])
    return _pad(x[:, None], 1)


def shared_border():
    """eps = 1, min_samples = 4, on a line.  Row 0 (x = 5) is core: {5, 6, 6, 4}; row 4 (x = 3) is core: {3, 2, 2, 4}; the rows
    at 6 and at 2 have 3 rows within eps: border.  Row 3 (x = 4) has {4, 5, 3}: not core, and a core row of BOTH clusters
    within eps — it takes the lower label.  Row 7 is noise."""
    return _pad(np.array([5, 6, 6, 4, 3, 2, 2, 100])[:, None], 2)


def border_before_core():
    """eps = 1, min_samples = 4, on a line.  Row 0 (x = 2) is a border row of the cluster whose only core row is row 5 (x = 3:
    {3, 2, 2, 4}); the cluster around row 1 (x = 50: {50, 51, 51, 49}) starts later than row 0 but its core row comes first:
    it is cluster 0, and row 0 carries label 1.  Row 8 is noise."""
    return _pad(np.array([2, 50, 51, 51, 49, 3, 2, 4, 200])[:, None], 2)


def crafted_cases():
    """{name: (table, k, eps, min_samples)}"""
    return {
        "blobs": (blobs(), 3, 1.0, 5),
        "chain": (chain(), 1, 1.0, 2),
        "shared_border": (shared_border(), 2, 1.0, 4),
        "border_before_core": (border_before_core(), 2, 1.0, 4),
        "min_samples_1": (blobs(), 3, 1.0, 1),     # every row is core: no lists, stride 0
        "min_samples_2": (blobs(), 3, 1.0, 2),     # a row with a neighbour is core: no border rows by construction
    }


# seeds under which the clusters come out in ANOTHER order than in the given row order (tests/test_clusters_host.py checks it)
PERMUTATION_SEEDS = {"blobs": 1, "chain": 6, "shared_border": 2, "border_before_core": 2, "min_samples_1": 1, "min_samples_2": 1}


def permutation(name, n):
    """the fixed random order the crafted set ``name`` is also run in"""
    return np.random.default_rng(PERMUTATION_SEEDS[name]).permutation(n)


# what the structure of a crafted set allows: min_samples = 1 makes every row core (no border, no noise); min_samples = 2
# makes every row with a neighbour core (no border)
def expects_border(min_samples):
    return min_samples > 2


def expects_noise(min_samples):
    return min_samples > 1


# ---- cosine ---------------------------------------------------------------------------------------
COSINE_EPS, COSINE_MIN_SAMPLES, COSINE_K = 0.05, 3, 8


def bundles():
    """four bundles of 70 directions (rows 0 .. 279, interleaved) around the axes e0 .. e3 of R^8, each row its axis plus a
    perturbation of at most 0.02 per coordinate, scaled by a length in [0.5, 4]; then the four axes e4 .. e7 once each.
    Two rows of a bundle are within an angle of 2 atan(0.02 sqrt 7) = 0.106: distance 1 - cos < 0.0057; rows of different
    bundles are at 1 - cos > 0.89 (|cos| < 2 * 0.053 + 0.053^2).  eps = 0.05 has a margin of 0.044 on either side — four
    orders of magnitude above the (2 k + 6) 2^-24 = 1.3e-6 of the f32 chain.  min_samples = 3: four clusters, four noise rows."""
    rng = np.random.default_rng(77)
    rows = []
    for t in range(70):
        for axis in range(4):
            v = rng.uniform(-0.02, 0.02, size=COSINE_K)
            v[axis] = 1.0
            rows.append(v * rng.uniform(0.5, 4.0))
    for axis in range(4, 8):
        v = np.zeros(COSINE_K)
        v[axis] = 2.0
        rows.append(v)
    return np.asarray(rows, F32)


def cosine_distances(X):
    X64 = X.astype(np.float64)
    N = X64 / np.sqrt((X64 * X64).sum(1))[:, None]
    return 1.0 - N @ N.T
