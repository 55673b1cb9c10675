"""emg_rows_dbscan on the GPU, on REAL-VALUED tables: labels, core flags and info against tests/_dbscan_ref.py over the
distances the contract defines (tests/_chain_ref.py: the k-ordered fmaf chains of oracle/emg_oracle.c).

tests/test_clusters.py runs the kernel on small integers, where any arithmetic gives the same distance bits.  Here eps is a
chain distance that OCCURS, chosen so that a row is core only because a pair lies exactly at eps: a distance that is one bit
off — another summation order, a Gram form, an unfused product — makes that row not core, or another row core, and the labels
differ.  Every comparison is an equality of labels, flags and counts."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from emgraph_amd import _lib as L  # noqa: E402
from tests import _chain_ref as ref  # noqa: E402
from tests._dbscan_ref import dbscan_ref, summary  # noqa: E402

F32 = np.float32
N_ROWS = (65, 257, 1000)
K_INT = (3, 33, 100, 400)
MIN_SAMPLES = (3, 5)
LAYOUTS = ("unpadded", "padded")


def dev():
    from emgraph_amd import device
    device.require_gpu()
    return device


def cuda(a):
    """a device table with NO row padding: at odd k the rows are not 16-byte aligned"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).cuda()


def padded(a):
    """the package's padded row layout"""
    from emgraph_amd.training import alloc_table
    return alloc_table(a.shape[0], a.shape[1], torch.device("cuda"), init=a)


def check(table_t, k, metric, eps, min_samples, expected, where):
    labels, core = expected
    g_labels, g_core, g_info = dev().rows_dbscan(table_t, k, metric, eps, min_samples)
    g_labels, g_core, g_info = g_labels.cpu().numpy(), g_core.cpu().numpy(), g_info.cpu().numpy()
    assert np.array_equal(g_core, core.astype(np.uint8)), where
    assert np.array_equal(g_labels, labels), where
    clusters, _, noise = summary(labels, core)
    assert g_info.tolist() == [clusters, noise], where


def exact_radius_cases(D, seed):
    """[(i, min_samples, eps)]: 4 seeded rows i for each min_samples m, eps the distance from row i to its (m - 1)-th nearest
    other row — with its own 0 the m-th smallest entry of row i — so row i is core only through a pair AT eps"""
    rng = np.random.default_rng(seed)
    return [(i, m, ref.core_eps(D, i, m)) for m in MIN_SAMPLES for i in rng.integers(0, len(D), 4).tolist()]


def run_cases(rows_in, D, k, metric, seed, where):
    """every case on the rows as given and on one seeded permutation of them (as test_dbscan_l2_crafted_sets); ``rows_in(order)``
    returns the device tables to run on, one per layout"""
    n = len(D)
    cases = exact_radius_cases(D, seed)
    for order in (np.arange(n), np.random.default_rng(seed + 1).permutation(n)):
        Do = D[np.ix_(order, order)]                 # the chain is a function of the pair: the permuted table's matrix
        tables = rows_in(order)
        for i, m, eps in cases:
            expected = dbscan_ref(ref.within_matrix(Do, eps), m)
            assert expected[1][np.nonzero(order == i)[0][0]]
            for name, t in tables:
                check(t, k, metric, eps, m, expected, "%s %s: n %d k %d row %d min_samples %d eps %r" % (where, name, n, k, i, m, eps))


@pytest.mark.parametrize("k", K_INT)
@pytest.mark.parametrize("n", N_ROWS)
def test_dbscan_l2_blobs_with_a_pair_exactly_at_eps(n, k):
    X = ref.blobs(n, k)
    D = ref.l2_chain(X, X)
    run_cases(lambda order: [("unpadded", cuda(X[order])), ("padded", padded(X[order]))], D, k, L.METRIC_L2, 7000 + n + k, "l2")


def test_dbscan_cosine_with_a_pair_exactly_at_eps():
    """the same construction on the rows the device normalised, with cosine_chain of exactly those rows"""
    d = dev()
    n, k = 257, 33
    X = ref.blobs(n, k)
    Nt = d.rows_normalize(cuda(X), k)
    N = Nt.cpu().numpy()
    D = ref.cosine_chain(N, N)

    def rows_in(order):
        idx = torch.from_numpy(order).cuda()
        sel = Nt.index_select(0, idx)                 # contiguous: ld = k
        assert np.array_equal(sel.cpu().numpy().view(np.int32), N[order].view(np.int32))
        return [("unpadded", sel), ("padded", padded(N[order]))]
    run_cases(rows_in, D, k, L.METRIC_COSINE, 7700, "cosine")


def test_dbscan_l2_nan_row():
    """a row holding a NaN is within eps of nothing: noise for min_samples > 1, a cluster of its own for min_samples = 1"""
    n, k = 257, 37
    X = ref.blobs(n, k)
    X[70, 36] = np.nan                                # in the k-tile tail
    X[256, 0] = np.nan                                # the last row: the one the tile stream clamps to
    D = ref.l2_chain(X, X)
    assert np.isnan(D[[70, 256]]).all() and np.isnan(D).sum() == 4 * n - 4
    clean = np.delete(np.arange(n), (70, 256))
    for m in (1, 3, 5):
        for i in (0, 7, 100):
            eps = ref.core_eps(D, i, max(m, 2))
            labels, core = dbscan_ref(ref.within_matrix(D, eps), m)
            if m == 1:
                assert core.all() and (np.bincount(labels)[labels[[70, 256]]] == 1).all()
            else:
                assert core[i] and (labels[[70, 256]] == -1).all() and not core[[70, 256]].any()
            # and the other rows are clustered as if the NaN rows were not there
            l2, c2 = dbscan_ref(ref.within_matrix(D[np.ix_(clean, clean)], eps), m)
            assert np.array_equal(c2, core[clean]) and np.array_equal(np.unique(l2, return_inverse=True)[1],
                                                                      np.unique(labels[clean], return_inverse=True)[1])
            for name, t in (("unpadded", cuda(X)), ("padded", padded(X))):
                check(t, k, L.METRIC_L2, eps, m, (labels, core), "nan %s: row %d min_samples %d eps %r" % (name, i, m, eps))
