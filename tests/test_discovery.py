"""Discovery on the GPU: the radius join emg_rows_within, emg_rows_normalize, and the two public functions.

l2 is checked BIT-EXACTLY: tables hold small integers in [-3, 3], so every squared distance is an integer that f32 holds
exactly whatever the summation order, and sqrtf of it is correctly rounded — the numpy brute force (Gram form on integers, exact
in float64) is the expected result to the bit, boundary ties (d == radius) included.  cosine is checked against float64 with
the bound derived below, the radius placed in a gap of the reference distances so that the pair SET must match exactly."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from emgraph_amd import _lib as L  # noqa: E402
from emgraph_amd import discovery  # noqa: E402
from emgraph_amd.models import ComplEx, TransE  # noqa: E402

F32 = np.float32
U = 2.0 ** -24
N_B = (1, 2, 63, 64, 65, 257, 1000)
K_INT = (1, 3, 4, 37, 100, 400)


def dev():
    from emgraph_amd import device
    device.require_gpu()
    return device


def cuda(a):
    """a device table with NO row padding: at k_int = 37 the rows are not 16-byte aligned"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).cuda()


def int_table(rng, n, k):
    """integers in [-3, 3]; a few rows are bit-identical copies of others (nearest-other ties, radius 0)"""
    B = rng.integers(-3, 4, size=(n, k)).astype(F32)
    if n >= 2:
        B[n - 1] = B[0]
    if n >= 63:
        B[40] = B[7]
        B[62] = B[7]
        B[5] = B[0]
    return B


def distances_l2(A, B):
    """(f32 distances, integer squared distances): small integers, so float64 products and sums are exact"""
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    d2 = (A64 * A64).sum(1)[:, None] + (B64 * B64).sum(1)[None, :] - 2 * (A64 @ B64.T)
    assert (d2 == np.rint(d2)).all() and d2.max(initial=0) < 2 ** 24
    return np.sqrt(d2.astype(F32)), d2          # exact integers below 2^24: the f32 square root is correctly rounded


def brute(dist, self_offset, radius):
    """(count, nn_dist, nn_id, sorted packed pairs) of the contract from the distance matrix"""
    n_a, n_b = dist.shape
    other = np.ones((n_a, n_b), bool)
    if self_offset >= 0:
        other[np.arange(n_a), self_offset + np.arange(n_a)] = False
    within = other & (dist <= F32(radius))
    masked = np.where(other, dist, F32(np.inf))
    nn_id = masked.argmin(1)                    # the first minimum: the lowest id
    nn_dist = masked[np.arange(n_a), nn_id].astype(F32)
    nn_id = np.where(other.any(1), nn_id, -1).astype(np.int32)
    i, j = np.nonzero(within)
    return within.sum(1).astype(np.int32), nn_dist, nn_id, np.sort((i.astype(np.int64) << 32) | j)


def brute_l2(A, B, self_offset, radius):
    return brute(distances_l2(A, B)[0], self_offset, radius)


def run_within(metric, A, B, k, self_offset, radius, cap=None, pairs=None):
    d = dev()
    count, nn_dist, nn_id, pairs, pc = d.rows_within(metric, A, B, k, self_offset, radius, pairs_capacity=cap, pairs=pairs)
    out = [count.cpu().numpy(), nn_dist.cpu().numpy(), nn_id.cpu().numpy()]
    if cap is None:
        return out + [None, None]
    pc = pc.cpu().numpy()
    return out + [pairs.cpu().numpy(), pc]


def check_l2(A, B, At, Bt, k, self_offset):
    dist, d2 = distances_l2(A, B)
    if self_offset >= 0:
        d2 = d2[~np.eye(A.shape[0], B.shape[0], self_offset, dtype=bool)]
    d2 = np.sort(d2.reshape(-1))
    radii = [0.0, float(np.sqrt(F32(d2[-1]))) + 1.0 if d2.size else 1.0]
    if d2.size:
        radii.append(float(np.sqrt(F32(d2[d2.size // 3]))))   # an m that occurs: pairs AT the radius count
    for radius in radii:
        count, nn_dist, nn_id, pairs = brute(dist, self_offset, radius)
        g_count, g_dist, g_id, _, _ = run_within(L.METRIC_L2, At, Bt, k, self_offset, radius)
        where = "n_a %d n_b %d k %d self %d radius %r" % (A.shape[0], B.shape[0], k, self_offset, radius)
        assert np.array_equal(g_count, count), where
        assert np.array_equal(g_dist.view(np.int32), nn_dist.view(np.int32)), where
        assert np.array_equal(g_id, nn_id), where
        g2 = run_within(L.METRIC_L2, At, Bt, k, self_offset, radius, cap=int(count.sum()))
        assert g2[4].tolist() == [int(count.sum()), 0], where
        assert np.array_equal(np.sort(g2[3][:len(pairs)]), pairs), where
        assert np.array_equal(g2[0], count) and np.array_equal(g2[2], nn_id), where


@pytest.mark.parametrize("n_b", N_B)
def test_within_l2_is_bit_exact(n_b):
    rng = np.random.default_rng(1000 + n_b)
    for k in K_INT:
        B = int_table(rng, n_b, k)
        Bt = cuda(B)
        check_l2(B, B, Bt, Bt, k, 0)                                   # the self-join
        n_s = min(5, n_b)
        off = n_b - n_s                                                # the slice straddles the last 64-row tile boundary
        check_l2(B[off:], B, Bt[off:], Bt, k, off)
        A = rng.integers(-3, 4, size=(7, k)).astype(F32)               # foreign rows, one of them equal to a row of B
        A[2] = B[n_b // 2]
        check_l2(A, B, cuda(A), Bt, k, -1)


def test_within_pair_buffer_overflow():
    rng = np.random.default_rng(7)
    n, k = 257, 4
    B = int_table(rng, n, k)
    Bt = cuda(B)
    radius = 3.0
    count, nn_dist, nn_id, pairs = brute_l2(B, B, 0, radius)
    total = int(count.sum())
    cap = total // 3
    assert cap > 64 and total > n
    GUARD = -0x0123456789abcdef
    buf = torch.full((cap + 16,), GUARD, dtype=torch.int64, device="cuda")
    g_count, g_dist, g_id, g_pairs, pc = run_within(L.METRIC_L2, Bt, Bt, k, 0, radius, cap=cap, pairs=buf)
    assert pc.tolist() == [cap, 1]
    assert np.array_equal(g_count, count) and np.array_equal(g_id, nn_id)
    assert np.array_equal(g_dist.view(np.int32), nn_dist.view(np.int32))
    assert (g_pairs[cap:] == GUARD).all(), "written past the capacity"
    wrote = g_pairs[:cap]
    assert len(np.unique(wrote)) == cap and np.isin(wrote, pairs).all()
    # the host's second pass: sized from the counts of the first
    again = run_within(L.METRIC_L2, Bt, Bt, k, 0, radius, cap=int(g_count.sum()))
    assert again[4].tolist() == [total, 0]
    assert np.array_equal(np.sort(again[3][:total]), pairs)


# ---- cosine -------------------------------------------------------------------------------------------
# Bounds, with u = 2^-24 the unit roundoff.  emg_rows_normalize is DEFINED as x / sqrtf(ss), ss the k-ordered f32 chain
# fmaf(x_k, x_k, ss): against a reference that follows that definition (the chain emulated step by step, square root and
# division in float64) the device adds the rounding of sqrtf and of the division, 2 u and second-order terms, so the
# specification's 4 u holds for every k and is asserted for every k (a chain in another order, or a sum of squares
# accumulated differently, moves ss by several of its ulps and the elements with it).  Against the PLAIN float64 normalisation
# the chain's own k roundings come on top — up to (k / 2 + 2) u — so 4 u cannot be promised for long rows; it is asserted
# where it holds, K_PLAIN_4U (figures: the test prints them; k = 37: 3.7 u, k = 100: 4.4 u, over the bound).
# Distance: each operand's elements are within (k / 2 + 2) u of the float64 unit row, which gives (k + 4) u sum|a b|
# <= (k + 4) u by Cauchy-Schwarz on unit rows; the dot chain adds k u, the subtraction from 1 at most 2 u on a result <= 2:
# (2 k + 6) u < (k + 8) 2^-23.
K_PLAIN_4U = (1, 3, 4, 37)


def chain_sum_of_squares(X):
    """the k-ordered f32 chain fmaf(x_k, x_k, ss) of every row: the product is exact in float64, the sum is rounded to f32
    once per step"""
    ss = np.zeros(len(X), F32)
    for c in range(X.shape[1]):
        x = X[:, c].astype(np.float64)
        ss = (x * x + ss.astype(np.float64)).astype(F32)
    return ss


def contract_reference(X):
    """x / sqrt(chain sum of squares), square root and division in float64; all-zero rows stay zero"""
    norm = np.sqrt(chain_sum_of_squares(X).astype(np.float64))
    X64 = X.astype(np.float64)
    return np.divide(X64, norm[:, None], out=np.zeros_like(X64), where=norm[:, None] > 0)


def cosine_reference(X):
    X64 = X.astype(np.float64)
    norm = np.sqrt((X64 * X64).sum(1))
    N = np.divide(X64, norm[:, None], out=np.zeros_like(X64), where=norm[:, None] > 0)
    return N, 1.0 - N @ N.T


@pytest.mark.parametrize("k", (1, 3, 4, 37, 100, 400))
def test_normalize_and_within_cosine(k):
    d = dev()
    rng = np.random.default_rng(50 + k)
    n = 257
    X = rng.standard_normal((n, k)).astype(F32)
    X[11] = 0.0                       # an all-zero row stays zero: its distance to everything is 1
    X[200] = X[3]                     # a duplicate
    X[201] = 2.5 * X[3]               # and a parallel row
    Xt = cuda(X)
    N, D = cosine_reference(X)
    Nt = d.rows_normalize(Xt, k)
    got = Nt.cpu().numpy().astype(np.float64)
    C = contract_reference(X)
    err_c, err_p = np.abs(got - C), np.abs(got - N)
    print("k %d: max element error %.3g u of the contract reference, %.3g u of plain float64 (bound 4 u)"
          % (k, (err_c / np.maximum(np.abs(C), 1e-300)).max() / U, (err_p / np.maximum(np.abs(N), 1e-300)).max() / U))
    assert (err_c <= 4 * U * np.abs(C)).all()
    if k in K_PLAIN_4U:
        assert (err_p <= 4 * U * np.abs(N)).all()
    assert (got[11] == 0).all()

    bound = (k + 8) * 2.0 ** -23
    off = D[~np.eye(n, dtype=bool)]
    srt = np.unique(off)
    gaps = np.nonzero(np.diff(srt) > 4 * bound)[0]   # the radius: the middle of the wide gap nearest the 5 % quantile
    g = int(gaps[np.argmin(np.abs(gaps - len(srt) // 20))])
    radius = float(F32((srt[g] + srt[g + 1]) / 2))
    assert (np.abs(off - radius) > bound).all(), "no gap wide enough for the radius"
    within = (D <= radius) & ~np.eye(n, dtype=bool)
    i, j = np.nonzero(within)
    pairs = np.sort((i.astype(np.int64) << 32) | j)
    assert len(pairs) >= 2            # (3, 200) at least
    g_count, g_dist, g_id, g_pairs, pc = run_within(L.METRIC_COSINE, Nt, Nt, k, 0, radius, cap=len(pairs) + 8)
    assert pc.tolist() == [len(pairs), 0]
    assert np.array_equal(np.sort(g_pairs[:len(pairs)]), pairs)
    assert np.array_equal(g_count, within.sum(1))
    masked = np.where(np.eye(n, dtype=bool), np.inf, D)
    print("k %d: max nearest-distance error %.3g (bound %.3g)" % (k, np.abs(g_dist - masked.min(1)).max(), bound))
    assert (np.abs(g_dist - masked.min(1)) <= bound).all()
    assert (masked[np.arange(n), g_id] <= masked.min(1) + 2 * bound).all()


# ---- the public functions ---------------------------------------------------------------------------------
def crafted(cls, ent, rel, k):
    """a fitted model whose parameters are the given arrays"""
    m = cls(k=k, epochs=1, batches_count=1)
    m.ent_to_idx = {"e%03d" % i: i for i in range(len(ent))}
    m.rel_to_idx = {"r%02d" % i: i for i in range(len(rel))}
    m.trained_model_params = [np.ascontiguousarray(ent, F32), np.ascontiguousarray(rel, F32)]
    m.is_fitted = True
    return m


@pytest.fixture(scope="module")
def planted():
    """integer tables with planted groups: entities {3, 17, 90} identical, 41 one step from 40 and 42 one step from 41
    (a chain: 40 and 42 are two steps apart); relations {1, 4} identical"""
    rng = np.random.default_rng(99)
    k = 6
    ent = rng.integers(-3, 4, size=(130, 2 * k)).astype(F32)
    ent[:, 0] = np.arange(130) * 4 % 7 - 3
    ent[17] = ent[3]
    ent[90] = ent[3]
    ent[40] = 0
    ent[41] = 0
    ent[42] = 0
    ent[40, :3] = (9, 9, 8)
    ent[41, :3] = (9, 9, 9)
    ent[42, :3] = (9, 9, 10)
    rel = rng.integers(-3, 4, size=(6, 2 * k)).astype(F32)
    rel[4] = rel[1]
    return ent, rel, k


def name_e(i):
    return "e%03d" % i


def host_neighbours(ent, q, cand, n):
    """ids and distance bits by the integer brute force, (distance, id) order, padded"""
    dist, _ = distances_l2(ent[q], ent[cand])
    ids = np.full((len(q), n), -1, np.int32)
    out = np.full((len(q), n), np.inf, F32)
    for r in range(len(q)):
        order = np.lexsort((cand, dist[r]))[:n]
        ids[r, :len(order)] = np.asarray(cand)[order]
        out[r, :len(order)] = dist[r][order]
    return ids, out


def test_find_nearest_neighbours(planted):
    ent, rel, k = planted
    m = crafted(ComplEx, ent, rel, k)                      # 2k columns: the whole row is the embedding
    q = [3, 40, 0, 129, 17]
    labels = [name_e(i) for i in q]
    # all entities
    ids, dist = discovery.find_nearest_neighbours(m, q, n_neighbors=10, from_idx=True)
    w_ids, w_dist = host_neighbours(ent, q, np.arange(130), 10)
    assert ids.dtype == np.int32 and dist.dtype == F32
    assert np.array_equal(ids, w_ids) and np.array_equal(dist.view(np.int32), w_dist.view(np.int32))
    assert ids[0, :3].tolist() == [3, 17, 90] and (dist[0, :3] == 0).all()   # itself first, then its copies by id
    nbr, dist2 = discovery.find_nearest_neighbours(m, labels, n_neighbors=10)
    assert nbr.dtype == object and nbr.tolist() == [[name_e(i) for i in row] for row in w_ids.tolist()]
    assert np.array_equal(dist2.view(np.int32), w_dist.view(np.int32))
    # a subset with a repeated label, and more neighbours asked for than it holds
    sub = [90, 5, 41, 5, 42, 128]
    cand = np.unique(sub)
    nbr, dist = discovery.find_nearest_neighbours(m, labels, n_neighbors=8, entities_subset=[name_e(i) for i in sub])
    w_ids, w_dist = host_neighbours(ent, q, cand, 8)
    assert (w_ids[:, 5:] == -1).all() and np.isinf(w_dist[:, 5:]).all()
    assert nbr.tolist() == [[None if i < 0 else name_e(i) for i in row] for row in w_ids.tolist()]
    assert np.array_equal(dist.view(np.int32), w_dist.view(np.int32))
    # cosine, within the bound of test_normalize_and_within_cosine
    _, D = cosine_reference(ent)
    ids, dist = discovery.find_nearest_neighbours(m, q, n_neighbors=12, metric="cosine", from_idx=True)
    bound = (2 * k + 8) * 2.0 ** -23
    for r, e in enumerate(q):
        want = np.sort(D[e])[:12]
        assert (np.abs(dist[r] - want) <= bound).all()
        assert (np.abs(D[e][ids[r]] - want) <= 2 * bound).all()        # the ids are entities at those distances
        assert (np.diff(dist[r]) >= 0).all() and len(set(ids[r].tolist())) == 12
    assert ids[0, :3].tolist() == [3, 17, 90]


def test_find_duplicates_returns_the_planted_neighbourhoods(planted):
    ent, rel, k = planted
    m = crafted(ComplEx, ent, rel, k)
    E = np.array([name_e(i) for i in range(130)])
    e = name_e
    identical = frozenset({e(3), e(17), e(90)})
    dups, tol = discovery.find_duplicates(E, m, mode="entity", metric="l2", tolerance=0.0)
    assert tol == 0.0 and dups == {identical}
    dups, tol = discovery.find_duplicates(E, m, tolerance=1.0)            # the chain 40 ~ 41 ~ 42: neighbourhoods
    assert tol == 1.0
    assert dups == {identical, frozenset({e(40), e(41)}), frozenset({e(40), e(41), e(42)}), frozenset({e(41), e(42)})}
    dups, _ = discovery.find_duplicates(E[[3, 40, 90, 41, 3]], m, tolerance=1.0)   # a selection, one label twice
    assert dups == {frozenset({e(3), e(90)}), frozenset({e(40), e(41)})}
    dups, _ = discovery.find_duplicates(E, m, metric="cosine", tolerance=1e-5)
    assert identical in dups and all(len(s) <= 3 for s in dups)
    R = np.array(["r%02d" % i for i in range(6)])
    dups, _ = discovery.find_duplicates(R, m, mode="relation", tolerance=0.0)
    assert dups == {frozenset({"r01", "r04"})}
    # triples: (s, p, o) rows concatenated — equal iff all three rows are
    T = np.array([[e(3), "r01", e(40)], [e(17), "r04", e(40)], [e(90), "r01", e(41)], [e(3), "r02", e(40)], [e(5), "r01", e(6)]])
    dups, _ = discovery.find_duplicates(T, m, mode="triple", tolerance=0.0)
    assert dups == {frozenset({tuple(T[0]), tuple(T[1])})}
    dups, _ = discovery.find_duplicates(T, m, mode="triple", tolerance=1.0)
    assert dups == {frozenset({tuple(T[0]), tuple(T[1]), tuple(T[2])})}
    # a real-valued model: k columns
    m2 = crafted(TransE, ent[:, :k], rel[:, :k], k)
    dups, _ = discovery.find_duplicates(E, m2, tolerance=0.0)
    assert identical in dups


def test_find_duplicates_auto_tolerance_is_the_quantile(planted):
    ent, rel, k = planted
    m = crafted(ComplEx, ent, rel, k)
    E = np.array([name_e(i) for i in range(130)])
    dist, _ = distances_l2(ent, ent)
    np.fill_diagonal(dist, np.inf)
    nn = dist.min(1)
    for f in (0.02, 0.1, 0.35):
        dups, tol = discovery.find_duplicates(E, m, tolerance="auto", expected_fraction_duplicates=f)
        want = np.sort(nn)[int(np.ceil(round(f * 130, 9))) - 1]
        assert F32(tol) == want
        assert (nn <= tol).mean() >= f
        smaller = nn[nn < tol]
        if len(smaller):
            assert (nn <= smaller.max()).mean() < f
        # and the result is the neighbourhood set at that tolerance
        within = dist <= F32(tol)
        assert dups == {frozenset([name_e(i)] + [name_e(j) for j in np.nonzero(within[i])[0]]) for i in range(130) if within[i].any()}
