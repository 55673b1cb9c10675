"""find_clusters on the GPU: the exact DBSCAN emg_rows_dbscan and the public function.

l2 is checked BIT-EXACTLY: the tables of tests/_dbscan_cases.py hold small integers, so every squared distance is an integer
that f32 holds exactly whatever the summation order and sqrtf of it is correctly rounded — which rows are within eps is known
exactly, pairs AT the radius included, and labels, core flags and info must equal those of tests/_dbscan_ref.py (DBSCAN from
its definition; tests/test_clusters_host.py pins it to scikit-learn).  cosine: bundles whose inside and outside distances are
0.044 away from eps (the f32 chain's error is below 2e-6), against float64 distances."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from emgraph_amd import _lib as L  # noqa: E402
from emgraph_amd import discovery  # noqa: E402
from emgraph_amd.models import ComplEx, TransE  # noqa: E402
from tests import _dbscan_cases as cases  # noqa: E402
from tests._dbscan_ref import dbscan_ref, summary  # noqa: E402

F32 = np.float32


def dev():
    from emgraph_amd import device
    device.require_gpu()
    return device


def cuda(a):
    """a device table with NO row padding: at k_int = 37 the rows are not 16-byte aligned"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).cuda()


def check(table_t, k, metric, eps, min_samples, within, where):
    labels, core = dbscan_ref(within, min_samples)
    g_labels, g_core, g_info = dev().rows_dbscan(table_t, k, metric, eps, min_samples)
    g_labels, g_core, g_info = g_labels.cpu().numpy(), g_core.cpu().numpy(), g_info.cpu().numpy()
    assert g_labels.dtype == np.int32 and g_core.dtype == np.uint8 and g_info.dtype == np.int64
    assert np.array_equal(g_core, core.astype(np.uint8)), where
    assert np.array_equal(g_labels, labels), where
    clusters, _, noise = summary(labels, core)
    assert g_info.tolist() == [clusters, noise], where


@pytest.mark.parametrize("n", cases.N_RANDOM)
def test_dbscan_l2_random_tables_are_bit_exact(n):
    for table, k, radii in cases.random_cases(n):
        t = cuda(table)
        dist = cases.distances_l2(table)[0]
        for m, eps in radii:
            within = dist <= F32(eps)
            for min_samples in cases.MIN_SAMPLES:
                check(t, k, L.METRIC_L2, eps, min_samples, within, "n %d k %d eps %r min_samples %d" % (n, k, eps, min_samples))


@pytest.mark.parametrize("name", sorted(cases.crafted_cases()))
def test_dbscan_l2_crafted_sets(name):
    table, k, eps, min_samples = cases.crafted_cases()[name]
    for order in (np.arange(len(table)), cases.permutation(name, len(table))):
        rows = table[order]
        check(cuda(rows), k, L.METRIC_L2, eps, min_samples, cases.within_l2(rows, eps), name)


def test_dbscan_cosine_bundles():
    X = cases.bundles()
    D64 = cases.cosine_distances(X)
    assert (np.abs(D64 - cases.COSINE_EPS) > 0.04).all()      # the margin; the f32 chain is within (2 k + 6) 2^-24 = 1.3e-6
    d = dev()
    rows = d.rows_normalize(cuda(X), cases.COSINE_K)
    check(rows, cases.COSINE_K, L.METRIC_COSINE, cases.COSINE_EPS, cases.COSINE_MIN_SAMPLES, D64 <= cases.COSINE_EPS, "cosine")
    order = cases.permutation("blobs", len(X))
    rows = d.rows_normalize(cuda(X[order]), cases.COSINE_K)
    check(rows, cases.COSINE_K, L.METRIC_COSINE, cases.COSINE_EPS, cases.COSINE_MIN_SAMPLES,
          D64[np.ix_(order, order)] <= cases.COSINE_EPS, "cosine, permuted")


def test_undersized_workspace_is_refused_and_nothing_is_launched():
    d = dev()
    lib = L.load()
    table, k, eps, min_samples = cases.crafted_cases()["shared_border"]
    n = len(table)
    t = cuda(table)
    need = d.rows_dbscan_ws_bytes(n, min_samples)
    assert need == lib.emg_rows_dbscan_ws_bytes(n, min_samples) > 28 * n
    assert lib.emg_rows_dbscan_ws_bytes(n, 0) == 0 and lib.emg_rows_dbscan_ws_bytes(-1, 5) == 0
    assert n % 4 == 0 and d.rows_dbscan_ws_bytes(n, min_samples + 1) == need + 4 * n      # one more list slot per row
    GUARD = -7
    labels = torch.full((n,), GUARD, dtype=torch.int32, device="cuda")
    core = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    info = torch.full((2,), GUARD, dtype=torch.int64, device="cuda")
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")

    def call(ws_bytes, eps=eps, min_samples=min_samples):
        return lib.emg_rows_dbscan(L.METRIC_L2, t.data_ptr(), n, t.stride(0), k, eps, min_samples, labels.data_ptr(),
                                   core.data_ptr(), info.data_ptr(), ws.data_ptr(), ws_bytes, None)

    for rc in (call(need - 1), call(0), call(need, eps=-1.0), call(need, eps=float("nan")), call(need, min_samples=0),
               lib.emg_rows_dbscan(7, t.data_ptr(), n, t.stride(0), k, eps, min_samples, labels.data_ptr(), core.data_ptr(),
                                   info.data_ptr(), ws.data_ptr(), need, None),
               lib.emg_rows_dbscan(L.METRIC_L2, t.data_ptr(), n, t.stride(0), k, eps, min_samples, labels.data_ptr(),
                                   core.data_ptr(), info.data_ptr(), ws.data_ptr() + 4, need, None)):
        assert rc != 0
    with pytest.raises(L.EmgError, match="workspace"):
        d.rows_dbscan(t, k, L.METRIC_L2, eps, min_samples, ws=ws[:need - 16])
    torch.cuda.synchronize()
    assert (labels == GUARD).all() and (core == 9).all() and (info == GUARD).all() and (ws == 0).all()
    assert call(need) == 0                                    # and the same buffers do when the size is right
    torch.cuda.synchronize()
    want, want_core = dbscan_ref(cases.within_l2(table, eps), min_samples)
    assert np.array_equal(labels.cpu().numpy(), want) and np.array_equal(core.cpu().numpy(), want_core.astype(np.uint8))
    # no rows: info = {0, 0}
    assert lib.emg_rows_dbscan(L.METRIC_L2, None, 0, k, k, eps, min_samples, None, None, info.data_ptr(), ws.data_ptr(), need,
                               None) == 0
    assert info.cpu().tolist() == [0, 0]


# ---- the public function ------------------------------------------------------------------------------
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
    """integer tables, random rows far apart (squared distances around 100) with planted groups: entities {3, 17, 90, 91, 92}
    identical, 40 one step from them, 41 one step from 40 (sqrt 2 from the five), {60, 61} identical; relations {1, 4}
    identical"""
    rng = np.random.default_rng(99)
    k = 6
    ent = rng.integers(-3, 4, size=(130, 2 * k)).astype(F32)
    ent[:, 0] = np.arange(130) * 4 % 7 - 3
    for i in (17, 90, 91, 92, 40, 41):
        ent[i] = ent[3]
    ent[40, 1] += 1
    ent[41, 1] += 1
    ent[41, 2] += 1
    ent[61] = ent[60]
    rel = rng.integers(-3, 4, size=(6, 2 * k)).astype(F32)
    rel[4] = rel[1]
    return ent, rel, k


def name_e(i):
    return "e%03d" % i


def expected(rows, eps, min_samples):
    return dbscan_ref(cases.within_l2(rows, eps), min_samples)[0]


def test_find_clusters_entities_relations_triples(planted):
    ent, rel, k = planted
    m = crafted(ComplEx, ent, rel, k)                      # 2k columns: the whole row is the embedding
    E = np.array([name_e(i) for i in range(130)])
    # defaults (eps 0.5, min_samples 5): the five identical rows are a cluster, everything else is noise
    got = discovery.find_clusters(E, m)
    assert got.dtype == np.int32 and got.shape == (130,)
    want = expected(ent, 0.5, 5)
    assert np.array_equal(got, want) and np.nonzero(want == 0)[0].tolist() == [3, 17, 90, 91, 92] and (want <= 0).all()
    # eps = 1: 40 joins as a core row, 41 as a border row (only 40 is within 1 of it)
    got = discovery.find_clusters(E, m, "dbscan", "entity", eps=1.0, min_samples=5)
    want = expected(ent, 1.0, 5)
    assert np.array_equal(got, want) and np.nonzero(want == 0)[0].tolist() == [3, 17, 40, 41, 90, 91, 92]
    # min_samples = 2: the pair {60, 61} is a cluster of its own, numbered after the one that starts at row 3
    got = discovery.find_clusters(E, m, eps=0.0, min_samples=2)
    want = expected(ent, 0.0, 2)
    assert np.array_equal(got, want) and want[60] == want[61] == 1 and want.max() == 1
    # a selection in another order, with a repeated label: rows are NOT de-duplicated — three times e003 and once e017 are
    # four identical rows, a cluster at min_samples = 4 (two rows after de-duplication would be noise)
    sel = [5, 3, 60, 3, 17, 3, 61]
    got = discovery.find_clusters(E[sel], m, eps=0.0, min_samples=4)
    assert np.array_equal(got, expected(ent[sel], 0.0, 4)) and got.tolist() == [-1, 0, -1, 0, 0, 0, -1]
    # cosine: identical rows are at distance 0 up to rounding, the random rows far from each other
    got = discovery.find_clusters(E, m, eps=1e-5, min_samples=5, metric="cosine")
    D64 = cases.cosine_distances(ent)
    assert (np.abs(D64 - 1e-5) > 5e-6).all()               # (2 k + 6) 2^-24 = 1.8e-6 for these 12 columns
    assert np.array_equal(got, dbscan_ref(D64 <= 1e-5, 5)[0]) and (got[[3, 17, 90, 91, 92]] == 0).all()
    # relations
    R = np.array(["r%02d" % i for i in range(6)])
    got = discovery.find_clusters(R, m, mode="relation", eps=0.0, min_samples=2)
    assert got.tolist() == [-1, 0, -1, -1, 0, -1]
    # triples: the s, p and o rows concatenated
    e = name_e
    T = np.array([[e(3), "r01", e(40)], [e(17), "r04", e(40)], [e(90), "r01", e(41)], [e(3), "r02", e(40)], [e(5), "r01", e(6)]])
    ids = [(3, 1, 40), (17, 4, 40), (90, 1, 41), (3, 2, 40), (5, 1, 6)]
    rows = np.stack([np.concatenate([ent[s], rel[p], ent[o]]) for s, p, o in ids])
    got = discovery.find_clusters(T, m, mode="triple", eps=0.0, min_samples=2)
    assert np.array_equal(got, expected(rows, 0.0, 2)) and got.tolist() == [0, 0, -1, -1, -1]
    got = discovery.find_clusters(T, m, mode="triple", eps=1.0, min_samples=2)
    assert np.array_equal(got, expected(rows, 1.0, 2)) and got.tolist() == [0, 0, 0, -1, -1]
    # a real-valued model: k columns
    m2 = crafted(TransE, ent[:, :k], rel[:, :k], k)
    got = discovery.find_clusters(E, m2, eps=1.0, min_samples=3)
    assert np.array_equal(got, expected(ent[:, :k], 1.0, 3)) and got[3] == 0


class Recorder:
    def fit_predict(self, emb):
        self.emb = emb
        return list(range(len(emb)))[::-1]


def test_find_clusters_hands_the_rows_to_a_fit_predict_object(planted):
    ent, rel, k = planted
    m = crafted(ComplEx, ent, rel, k)
    X = np.array([name_e(i) for i in (7, 3, 7, 129)])
    rec = Recorder()
    got = discovery.find_clusters(X, m, rec)
    assert isinstance(got, np.ndarray) and got.tolist() == [3, 2, 1, 0]
    assert isinstance(rec.emb, np.ndarray) and rec.emb.shape == (4, 2 * k) and rec.emb.dtype == F32
    assert np.array_equal(rec.emb, m.get_embeddings(X, embedding_type="entity"))
    T = np.array([[name_e(3), "r01", name_e(40)], [name_e(5), "r00", name_e(6)]])
    got = discovery.find_clusters(T, m, rec, mode="triple")
    assert got.tolist() == [1, 0] and rec.emb.shape == (2, 6 * k)
    assert np.array_equal(rec.emb[1], np.concatenate([ent[5], rel[0], ent[6]]))
