"""Discovery on the GPU, on REAL-VALUED tables: the radius join, the nearest neighbours and the public functions against the
distances the contract DEFINES — sqrtf of the k-ordered chain fmaf(d, d, acc) for l2, 1 - the k-ordered chain
fmaf(a_k, b_k, acc) for cosine — computed on the host by tests/_chain_ref.py from oracle/emg_oracle.c::orc_chain_score.

tests/test_discovery.py runs the same kernels on small integers, where every summation order, the Gram form, an unfused
product and a k-tile tail with a step too many all give the same bits.  Here the tables are floats of the magnitude of real
embeddings, on which those arithmetics differ from the chain in a third to all of the pairs (tests/test_chain_ref_host.py),
and every comparison is an equality of bits, ids, sets or labels: there is no tolerance in this file."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from emgraph_amd import _lib as L  # noqa: E402
from emgraph_amd import discovery  # noqa: E402
from emgraph_amd.models import ComplEx, TransE  # noqa: E402
from tests import _chain_ref as ref  # noqa: E402
from tests._dbscan_ref import dbscan_ref  # noqa: E402

F32 = np.float32
K_INT = (1, 3, 4, 31, 32, 33, 37, 64, 100, 400)      # around TK = 32, an exact multiple, the unaligned 33 and 37
N_B = (1, 2, 63, 64, 65, 257)
K_AT_1000 = (33, 400)
LAYOUTS = ("unpadded", "padded")


def dev():
    from emgraph_amd import device
    device.require_gpu()
    return device


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


def cuda(a):
    """a device table with NO row padding: at odd k the rows are not 16-byte aligned (the scalar loads)"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).cuda()


def padded(a):
    """the package's padded row layout"""
    from emgraph_amd.training import alloc_table
    return alloc_table(a.shape[0], a.shape[1], torch.device("cuda"), init=a)


def strided(a, ld):
    """a device table whose row stride is ``ld`` floats, the columns past k filled with NaN: nothing may read them"""
    buf = torch.full((a.shape[0], ld), float("nan"), dtype=torch.float32, device="cuda")
    view = buf[:, :a.shape[1]]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=F32)))
    return view


def on_device(a, layout):
    return cuda(a) if layout == "unpadded" else padded(a)


def foreign(a, Bt):
    """the foreign rows, in a layout whose ld differs from B's"""
    At = strided(a, Bt.stride(0) + 3)
    assert At.stride(0) != Bt.stride(0)
    return At


def radii_of(dist, self_offset):
    """0, one past the largest distance, a distance that occurs at about the 5 % quantile (pairs AT the radius count) and the
    smallest positive distance — of the distances to OTHER rows that are numbers"""
    d = dist[ref.others(dist.shape[0], dist.shape[1], self_offset)]
    d = np.sort(d[~np.isnan(d)])
    if d.size == 0:
        return [0.0, 1.0]
    radii = [0.0, float(d[-1]) + 1.0, float(d[d.size // 20])]
    if (d > 0).any():
        radii.append(float(d[d > 0][0]))
    return radii


def run_within(metric, A, B, k, self_offset, radius, cap=None):
    count, nn_dist, nn_id, pairs, pc = dev().rows_within(metric, A, B, k, self_offset, radius, pairs_capacity=cap)
    out = [count.cpu().numpy(), nn_dist.cpu().numpy(), nn_id.cpu().numpy()]
    if cap is None:
        return out + [None, None]
    return out + [pairs.cpu().numpy(), pc.cpu().numpy()]


def check_join(metric, dist, At, Bt, k, self_offset, where):
    """the join of At with Bt at every radius of radii_of against the brute force over ``dist``"""
    assert dist.shape == (At.shape[0], Bt.shape[0])
    for radius in radii_of(dist, self_offset):
        count, nn_dist, nn_id, pairs = ref.brute(dist, self_offset, radius)
        at = "%s: n_a %d n_b %d k %d ld_a %d ld_b %d self %d radius %r" % (where, At.shape[0], Bt.shape[0], k, At.stride(0),
                                                                            Bt.stride(0), self_offset, radius)
        g_count, g_dist, g_id, _, _ = run_within(metric, At, Bt, k, self_offset, radius)
        assert np.array_equal(g_count, count), at
        assert np.array_equal(bits(g_dist), bits(nn_dist)), at
        assert np.array_equal(g_id, nn_id), at
        total = int(count.sum())
        g2 = run_within(metric, At, Bt, k, self_offset, radius, cap=total)
        assert g2[4].tolist() == [total, 0], at
        assert np.array_equal(np.sort(g2[3][:total]), pairs), at
        assert np.array_equal(g2[0], count) and np.array_equal(bits(g2[1]), bits(nn_dist)) and np.array_equal(g2[2], nn_id), at


def three_joins(metric, B, A, dist_bb, dist_ab, Bt, At, k, where):
    """the self-join, a slice straddling the last 64-row tile, and the foreign rows (as test_within_l2_is_bit_exact)"""
    n_b = B.shape[0]
    check_join(metric, dist_bb, Bt, Bt, k, 0, where)
    off = n_b - min(5, n_b)
    check_join(metric, dist_bb[off:], Bt[off:], Bt, k, off, where)
    check_join(metric, dist_ab, At, Bt, k, -1, where)


def foreign_rows(maker, B, k):
    """7 foreign rows from the same maker (another seed), one of them a copy of a row of B"""
    A = np.ascontiguousarray(ref.MAKERS[maker](7, k, seed=1))
    A[2] = B[B.shape[0] // 2]
    return A


def l2_shape(maker, n_b, k):
    B = ref.MAKERS[maker](n_b, k)
    A = foreign_rows(maker, B, k)
    dist_bb, dist_ab = ref.l2_chain(B, B), ref.l2_chain(A, B)
    for layout in LAYOUTS:
        Bt = on_device(B, layout)
        three_joins(L.METRIC_L2, B, A, dist_bb, dist_ab, Bt, foreign(A, Bt), k, "%s l2 %s" % (maker, layout))


@pytest.mark.parametrize("maker", sorted(ref.MAKERS))
@pytest.mark.parametrize("n_b", N_B)
def test_within_l2_has_the_bits_of_the_chain(n_b, maker):
    for k in K_INT:
        l2_shape(maker, n_b, k)


@pytest.mark.parametrize("maker", sorted(ref.MAKERS))
@pytest.mark.parametrize("k", K_AT_1000)
def test_within_l2_has_the_bits_of_the_chain_at_1000_rows(k, maker):
    l2_shape(maker, 1000, k)


def cosine_shape(n_b, k):
    """normal(1.0) through rows_normalize; the expected distances are cosine_chain of the DEVICE's normalised rows"""
    d = dev()
    X = ref.normal(n_b, k, scale=1.0)
    Y = np.ascontiguousarray(ref.normal(7, k, scale=1.0, seed=1))
    Y[2] = X[n_b // 2]
    NBt, NAt = d.rows_normalize(cuda(X), k), d.rows_normalize(cuda(Y), k)
    NB, NA = NBt.cpu().numpy(), NAt.cpu().numpy()
    assert np.array_equal(bits(NA[2]), bits(NB[n_b // 2]))
    dist_bb, dist_ab = ref.cosine_chain(NB, NB), ref.cosine_chain(NA, NB)
    for layout in LAYOUTS:
        Bt = NBt if layout == "padded" else cuda(NB)
        assert n_b == 1 or Bt.stride(0) == (k if layout == "unpadded" else (k + 3) // 4 * 4)
        three_joins(L.METRIC_COSINE, NB, NA, dist_bb, dist_ab, Bt, foreign(NA, Bt), k, "cosine %s" % layout)


@pytest.mark.parametrize("n_b", N_B)
def test_within_cosine_has_the_bits_of_the_chain(n_b):
    for k in K_INT:
        cosine_shape(n_b, k)


@pytest.mark.parametrize("k", K_AT_1000)
def test_within_cosine_has_the_bits_of_the_chain_at_1000_rows(k):
    cosine_shape(1000, k)


# ---- edge tables: l2, k = 37, n = 65; the expected values come from the same helper, nothing is special-cased ------------
EDGE_N, EDGE_K = 65, 37


def edge_case(B, must):
    A = np.ascontiguousarray(B[[3, 11, 20, 33, 47, 58, 64]] * F32(0.75))
    A[2] = B[EDGE_N // 2]
    dist_bb, dist_ab = ref.l2_chain(B, B), ref.l2_chain(A, B)
    must(dist_bb)
    for layout in LAYOUTS:
        Bt = on_device(B, layout)
        three_joins(L.METRIC_L2, B, A, dist_bb, dist_ab, Bt, foreign(A, Bt), EDGE_K, "edge l2 %s" % layout)
    return dist_bb


def test_within_l2_subnormal_squares():
    """a table scaled to 1e-19: the squares are near 1e-38, partly subnormal (f32's smallest normal is 1.18e-38)"""
    B = ref.normal(EDGE_N, EDGE_K, scale=1e-19)
    d = (B[:, None, :].astype(np.float64) - B[None, :, :]) ** 2
    tiny = float(np.finfo(F32).tiny)
    assert ((d > 0) & (d < tiny)).mean() > 0.2 and (d > tiny).mean() > 0.2

    def must(dist):
        off = dist[~np.eye(EDGE_N, dtype=bool)]
        assert np.isfinite(off).all() and (off > 0).mean() > 0.9
    edge_case(B, must)


def test_within_l2_overflowing_sums():
    """a table scaled to 3e18: sums of squares overflow.  A distance of +inf is within no finite radius, and the nearest row of
    a row that is at +inf from every other is the lowest other id, at distance inf."""
    B = ref.normal(EDGE_N, EDGE_K, scale=3e18)
    B[12] *= F32(4)                                   # and one row at +inf from EVERY other row

    def must(dist):
        off = dist[~np.eye(EDGE_N, dtype=bool)]
        assert np.isposinf(off).mean() > 0.5 and np.isfinite(off).sum() > 20 and not np.isnan(dist).any()
        assert np.isposinf(np.delete(dist[12], 12)).all()
    dist = edge_case(B, must)
    count, nn_dist, nn_id, _ = ref.brute(dist, 0, float(np.finfo(F32).max))
    assert count[12] == 0 and np.isposinf(nn_dist[12]) and nn_id[12] == 0


def test_within_l2_nan_rows():
    """two rows holding a NaN (one of them the table's last row, the one the tile stream clamps to): they are within nothing,
    nobody's nearest row, their own result is count 0 and (inf, -1), and they are in no pair"""
    B = ref.normal(EDGE_N, EDGE_K)
    B[3, 36] = np.nan                                 # in the k-tile tail
    B[64, 0] = np.nan

    def must(dist):
        assert np.isnan(dist[[3, 64]]).all() and np.isnan(dist[:, [3, 64]]).all() and np.isnan(dist).sum() == 4 * EDGE_N - 4
    dist = edge_case(B, must)
    count, nn_dist, nn_id, pairs = ref.brute(dist, 0, 10.0)
    assert count[[3, 64]].tolist() == [0, 0] and nn_id[[3, 64]].tolist() == [-1, -1] and np.isposinf(nn_dist[[3, 64]]).all()
    assert not np.isin(nn_id, (3, 64)).any() and not np.isin(pairs >> 32, (3, 64)).any() and not np.isin(pairs & 0xffffffff, (3, 64)).any()
    assert (count[np.setdiff1d(np.arange(EDGE_N), (3, 64))] == EDGE_N - 3).all()


# ---- one distance, one set of bits, across kernels ----------------------------------------------------------
@pytest.mark.parametrize("n,k", ((257, 100), (700, 37)))     # 700 rows: the 256-candidate chunk boundary of top-N is crossed
def test_every_kernel_gives_a_pair_the_same_distance(n, k):
    d = dev()
    X = ref.normal(n, k)
    Xt = padded(X)
    D = ref.l2_chain(X, X)
    _, w_dist, w_id, _ = ref.brute(D, 0, 0.0)
    # 1. the radius join
    _, g_dist, g_id, _, _ = run_within(L.METRIC_L2, Xt, Xt, k, 0, 0.0)
    assert np.array_equal(bits(g_dist), bits(w_dist)) and np.array_equal(g_id, w_id)
    # 2. top-N: every row is its own candidate too, so the five neighbours hold the row itself; the nearest OTHER row is the
    # first entry that is not the row
    ids, dist = discovery.neighbours_device(Xt, k, np.arange(n), 5, L.METRIC_L2)
    w_ids, w_d5 = ref.neighbours(D, np.arange(n), 5)
    assert np.array_equal(ids, w_ids) and np.array_equal(bits(dist), bits(w_d5))
    assert ids[n - 1, :2].tolist() == [0, n - 1] and ids[0, :2].tolist() == [0, n - 1]     # the planted tie: by id
    assert ids[62, :3].tolist() == [7, 40, 62] and (dist[62, :3] == 0).all()
    is_self = ids == np.arange(n)[:, None]
    assert (is_self.sum(1) == 1).all()
    first = np.argmin(is_self, axis=1)               # the first column that is not the row itself
    assert np.array_equal(ids[np.arange(n), first], w_id) and np.array_equal(bits(dist[np.arange(n), first]), bits(w_dist))
    # 3. the dense 1-vs-all scores
    S = -d.eval_scores_dense(L.TRANSE_L2, Xt, Xt, k, 1.0).cpu().numpy()
    assert np.array_equal(bits(S), bits(D))
    np.fill_diagonal(S, np.inf)
    assert np.array_equal(S.argmin(1), w_id) and np.array_equal(bits(S.min(1)), bits(w_dist))


# ---- the public functions on real-valued models -------------------------------------------------------------
N_ENT, N_REL = 130, 40


def crafted(cls, ent, rel, k):
    """a fitted model whose parameters are the given arrays"""
    m = cls(k=k, epochs=1, batches_count=1)
    m.ent_to_idx = {"e%03d" % i: i for i in range(len(ent))}
    m.rel_to_idx = {"r%02d" % i: i for i in range(len(rel))}
    m.trained_model_params = [np.ascontiguousarray(ent, F32), np.ascontiguousarray(rel, F32)]
    m.is_fitted = True
    return m


def name_e(i):
    return "e%03d" % i


def name_r(i):
    return "r%02d" % i


@pytest.fixture(scope="module", params=(("ComplEx", 6), ("TransE", 33)), ids=("ComplEx-6", "TransE-33"))
def real_model(request):
    """(model, ent, rel): blobs tables, ComplEx's rows are the whole 2k columns"""
    name, k = request.param
    cls, ki = (ComplEx, 2 * k) if name == "ComplEx" else (TransE, k)
    ent, rel = ref.blobs(N_ENT, ki), ref.blobs(N_REL, ki, seed=1)
    m = crafted(cls, ent, rel, k)
    assert m.internal_k == ki
    return m, ent, rel


def test_find_nearest_neighbours_real(real_model):
    m, ent, rel = real_model
    q = [3, 40, 0, 129, 7, 5, 9]
    w_ids, w_dist = ref.neighbours(ref.l2_chain(ent[q], ent), np.arange(N_ENT), 10)
    ids, dist = discovery.find_nearest_neighbours(m, q, n_neighbors=10, from_idx=True)
    assert ids.dtype == np.int32 and dist.dtype == F32
    assert np.array_equal(ids, w_ids) and np.array_equal(bits(dist), bits(w_dist))
    assert ids[1, :3].tolist() == [7, 40, 62] and ids[5, :2].tolist() == [5, 3]
    nbr, dist = discovery.find_nearest_neighbours(m, [name_e(i) for i in q], n_neighbors=10)
    assert nbr.tolist() == [[name_e(i) for i in row] for row in w_ids.tolist()] and np.array_equal(bits(dist), bits(w_dist))
    sub = [90, 5, 41, 5, 3, 128, 40, 62]
    cand = np.unique(sub)
    w_ids, w_dist = ref.neighbours(ref.l2_chain(ent[q], ent[cand]), cand, 8)
    ids, dist = discovery.find_nearest_neighbours(m, q, n_neighbors=8, entities_subset=sub, from_idx=True)
    assert np.array_equal(ids, w_ids) and np.array_equal(bits(dist), bits(w_dist)) and (ids[:, 7] == -1).all()


def test_find_duplicates_auto_tolerance_real(real_model):
    m, ent, rel = real_model
    E = np.array([name_e(i) for i in range(N_ENT)])
    D = ref.l2_chain(ent, ent)
    _, nn, _, _ = ref.brute(D, 0, 0.0)
    for f in (0.02, 0.05, 0.1, 0.35):
        dups, tol = discovery.find_duplicates(E, m, tolerance="auto", expected_fraction_duplicates=f)
        assert tol == discovery.auto_tolerance(nn, f)
        _, _, _, pairs = ref.brute(D, 0, tol)
        assert len(pairs) and dups == discovery.neighbourhoods(pairs, N_ENT, E.tolist())
    R = np.array([name_r(i) for i in range(N_REL)])
    Dr = ref.l2_chain(rel, rel)
    dups, tol = discovery.find_duplicates(R, m, mode="relation", tolerance="auto", expected_fraction_duplicates=0.2)
    assert tol == discovery.auto_tolerance(ref.brute(Dr, 0, 0.0)[1], 0.2)
    assert dups == discovery.neighbourhoods(ref.brute(Dr, 0, tol)[3], N_REL, R.tolist())


def test_find_clusters_real(real_model):
    """eps is the distance from a seeded row to its (m - 1)-th nearest other row over the rows _gather_rows defines, so that row
    is core only through a pair lying exactly at eps"""
    m, ent, rel = real_model
    rng = np.random.default_rng(21)
    sel = rng.permutation(N_ENT)[:100]
    sel[17] = sel[3]                                  # a label given twice is two rows
    spo = np.stack([rng.integers(0, N_ENT, 90), rng.integers(0, N_REL, 90), rng.integers(0, N_ENT, 90)], 1)
    spo[50:70, 1:] = spo[10:30, 1:]                   # triples that share two of their three rows
    spo[70:80] = spo[:10]
    spo[70:80, 0] = (spo[:10, 0] + 1) % N_ENT
    modes = {
        "entity": (np.array([name_e(i) for i in sel]), ent[sel]),
        "relation": (np.array([name_r(i) for i in range(N_REL)]), rel),
        "triple": (np.array([[name_e(s), name_r(p), name_e(o)] for s, p, o in spo]),
                   np.concatenate([ent[spo[:, 0]], rel[spo[:, 1]], ent[spo[:, 2]]], axis=1)),
    }
    for mode, (X, rows) in modes.items():
        D = ref.l2_chain(rows, rows)
        for min_samples in (3, 5):
            for i in rng.integers(0, len(rows), 4).tolist():
                eps = ref.core_eps(D, i, min_samples)
                labels, core = dbscan_ref(ref.within_matrix(D, eps), min_samples)
                assert core[i]
                got = discovery.find_clusters(X, m, mode=mode, eps=eps, min_samples=min_samples)
                assert got.dtype == np.int32 and np.array_equal(got, labels), "%s row %d min_samples %d" % (mode, i, min_samples)
