"""k-means on the GPU: emg_rows_kmeans, emg_rows_kmeans_seed and emgraph_amd.discovery.KMeans against tests/_kmeans_ref.py.

The contract fixes every bit (include/emgraph_hip.h, DESIGN.md 4.4 "k-means"): distances are the module's l2 chain, ties take
the lower index, means are f64 sums in a fixed order.  So labels, centres and n_iter are compared TO THE BIT, on integer tables
(every tie exact) and on real-valued ones (where another order of summation shows).  The inertia's order is the device's own:
it is compared within n 2^-52 relative, the bound of two f64 sums of n non-negative terms."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from emgraph_amd import _lib as L  # noqa: E402
from emgraph_amd import discovery  # noqa: E402
from emgraph_amd.models import ComplEx, DistMult  # noqa: E402
from tests import _chain_ref as cr  # noqa: E402
from tests import _kmeans_cases as cases  # noqa: E402
from tests import _kmeans_ref as R  # noqa: E402

F32 = np.float32


def dev():
    from emgraph_amd import device
    device.require_gpu()
    return device


def cuda(a):
    """a device table with NO row padding"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).cuda()


def padded(a, pad=3):
    """the same rows with a leading dimension that is no multiple of 4 floats, NaN in the padding"""
    a = np.ascontiguousarray(a, dtype=F32)
    buf = torch.full((a.shape[0], a.shape[1] + pad), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :a.shape[1]] = torch.from_numpy(a).cuda()
    return buf[:, :a.shape[1]]


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def run_device(Xt, k, start, max_iter, tol):
    d = dev()
    centres = cuda(start)
    labels, info = d.rows_kmeans(Xt, k, centres, max_iter, tol)
    inertia, n_iter, converged, tol_abs = d.kmeans_info(info)
    return labels.cpu().numpy(), centres.cpu().numpy(), inertia, n_iter, converged, tol_abs


def check(X, start, max_iter, tol, where, layouts=(cuda, padded)):
    """the device run equals the reference run; returns the reference's record"""
    ref = R.lloyd(X, start, max_iter, tol)
    n, k = X.shape
    for layout in layouts:
        got = run_device(layout(X), k, start, max_iter, tol)
        again = run_device(layout(X), k, start, max_iter, tol)
        labels, centres, inertia, n_iter, converged, tol_abs = got
        print("%s [%s]: n_iter %d/%d stopped_by %s inertia %r / %r tol_abs %r / %r" % (
            where, layout.__name__, n_iter, ref["n_iter"], ref["stopped_by"], inertia, ref["inertia"], tol_abs, ref["tol_abs"]))
        assert labels.dtype == np.int32 and centres.dtype == F32
        assert np.array_equal(labels, ref["labels"]), where
        assert np.array_equal(bits(centres), bits(ref["centres"])), where
        assert (n_iter, converged) == (ref["n_iter"], ref["converged"]), where
        assert abs(inertia - ref["inertia"]) <= n * 2.0 ** -52 * ref["inertia"], where
        # the variance's order is the reference's own (chunks of 256 rows): the same bits; a NaN in the table gives a NaN
        assert tol_abs == ref["tol_abs"] or (np.isnan(tol_abs) and np.isnan(ref["tol_abs"])), where
        # two runs: the same bits, the inertia included
        assert np.array_equal(again[0], labels) and np.array_equal(bits(again[1]), bits(centres)), where
        assert again[2:5] == got[2:5] and (again[5] == tol_abs or np.isnan(tol_abs)), where
    return ref


@pytest.mark.parametrize("n,k,C", cases.SHAPES)
def test_lloyd_equals_the_reference_to_the_bit(n, k, C):
    for name, X in cases.tables(n, k).items():
        start = X[cases.start_rows(n, C)]
        check(X, start, cases.MAX_ITER, 0.0, "%s n %d k %d C %d" % (name, n, k, C))


@pytest.mark.parametrize("name", sorted(cases.SIZED))
def test_cluster_sizes_around_the_chunk_length(name):
    sizes = cases.SIZED[name]
    X, start, owner = cases.sized_clusters(sizes)
    ref = check(X, start, cases.MAX_ITER, 0.0, name)
    assert np.array_equal(ref["labels"], owner) and np.bincount(ref["labels"]).tolist() == sizes and ref["n_iter"] == 1


def test_nan_row_gets_no_label_and_joins_nothing():
    X = cr.blobs(257, 33)
    X[100, 7] = np.nan
    X[256, :] = np.nan
    start = X[[0, 1, 2, 3, 50, 60]]
    ref = check(X, start, cases.MAX_ITER, 0.0, "nan rows")
    assert ref["labels"][100] == ref["labels"][256] == -1 and (np.delete(ref["labels"], [100, 256]) >= 0).all()
    assert np.isfinite(ref["centres"]).all() and np.isfinite(ref["inertia"]) and np.isnan(ref["tol_abs"])
    # a NaN centre is no candidate for anybody; with every centre NaN every row is unlabelled and the inertia is 0
    start = X[[0, 100, 2]]
    ref = check(X, start, 5, 0.0, "nan centre")
    assert not (ref["labels"] == 1).any() and np.isnan(ref["centres"][1]).any()
    ref = check(X, X[[100, 256]], 3, 0.0, "nan centres only")
    assert (ref["labels"] == -1).all() and ref["inertia"] == 0.0 and ref["n_iter"] == 1


def test_empty_cluster_keeps_its_centre():
    X = cr.normal(130, 40)                                   # rows 0 and 129 are identical
    start = X[[0, 5, 129, 77]]
    first, _, _ = R.assign(X, start)
    assert not (first == 2).any() and first[0] == first[129] == 0          # the tie goes to the lower index: cluster 2 is empty
    ref = check(X, start, 1, 0.0, "two equal centres, one update")
    assert ref["min_count"] == 0 and np.array_equal(bits(ref["centres"][2]), bits(X[129]))
    assert np.nonzero(ref["labels"] == 2)[0].tolist() == [0, 129]          # centre 0 moved away, the kept centre takes them
    ref = check(X, start, cases.MAX_ITER, 0.0, "two equal centres")
    assert ref["min_count"] == 0 and ref["stopped_by"] == "labels" and ref["n_iter"] > 1
    X = cases.integers(1000, 1)                              # 7 different values, 20 centres
    ref = check(X, X[cases.start_rows(1000, 20)], cases.MAX_ITER, 0.0, "more centres than values")
    assert ref["min_count"] == 0 and len(np.unique(ref["labels"])) <= 7


def test_tol_stop_with_a_margin():
    X, start, tol = cases.tol_case()
    ref = check(X, start, 100, tol, "tol stop")
    assert ref["stopped_by"] == "tol" and ref["stop_margin"] > 1e-3 and ref["near_tol"] > 1e-3
    # (an f64 sum of C k = 240 squares in another order moves the shift by 240 2^-53 relative at most)


def test_max_iter_zero_is_predict_and_max_iter_exhausted_is_consistent():
    X, start, _ = cases.tol_case()
    n, k = X.shape
    ref0 = check(X, start, 0, 0.0, "max_iter 0")
    labels0, _, _ = R.assign(X, start)
    assert np.array_equal(ref0["labels"], labels0) and ref0["n_iter"] == 0 and not ref0["converged"]
    assert np.array_equal(bits(ref0["centres"]), bits(start))
    ref2 = check(X, start, 2, 0.0, "max_iter 2")
    assert ref2["stopped_by"] == "max_iter" and ref2["n_iter"] == 2 and not ref2["converged"]
    labels2, dist2, _ = R.assign(X, ref2["centres"])
    assert np.array_equal(ref2["labels"], labels2) and ref2["inertia"] == R.inertia_of(labels2, dist2)
    # the estimator's predict is the max_iter = 0 run
    km = discovery.KMeans(len(start), init=start, max_iter=2, tol=0.0)
    assert np.array_equal(km.fit_predict(X), ref2["labels"]) and km.n_iter_ == 2
    assert np.array_equal(bits(km.cluster_centers_), bits(ref2["centres"]))
    other = cr.mixed(130, k)
    want, _, _ = R.assign(other, ref2["centres"])
    got = km.predict(cuda(other))
    assert got.dtype == np.int32 and np.array_equal(got, want) and np.array_equal(km.predict(other), want)


@pytest.mark.parametrize("maker,n,k,C,seed", cases.SEED_CASES)
def test_seeding_picks_the_reference_rows(maker, n, k, C, seed):
    d = dev()
    X = cases.integers(n, k) if maker == "integers" else cr.MAKERS[maker](n, k)
    for restart in range(3):
        first, u = R.draws(seed, restart, n, C, "k-means++")
        chosen, centres, margin = R.seed(X, C, first, u)
        for layout in (cuda, padded):
            g_centres, g_chosen = d.rows_kmeans_seed(layout(X), k, C, first, u)
            print("seeding %s n %d C %d restart %d: pick margin %.3g" % (maker, n, C, restart, margin))
            assert np.array_equal(g_chosen.cpu().numpy(), chosen), (maker, restart)
            assert np.array_equal(bits(g_centres.cpu().numpy()), bits(centres))


def test_seeding_when_all_rows_coincide():
    d = dev()
    X = np.tile(cr.normal(3, 33)[1], (300, 1))
    first, u = 17, np.array([0.0, 0.5, 0.999, 0.125, 0.25])
    chosen, centres, margin = R.seed(X, 6, first, u)
    assert chosen.tolist() == [17, 0, 150, 299, 37, 75] and margin == np.inf      # S_n = 0: floor(u n)
    g_centres, g_chosen = d.rows_kmeans_seed(cuda(X), 33, 6, first, u)
    assert g_chosen.cpu().tolist() == chosen.tolist() and np.array_equal(bits(g_centres.cpu().numpy()), bits(centres))
    # all but one row coincide: once the odd row and a common row are taken, S_n = 0
    X[123] += F32(1.0)
    chosen, _, _ = R.seed(X, 4, 5, np.array([0.3, 0.75, 0.5]))
    assert chosen.tolist() == [5, 123, 225, 150]
    assert d.rows_kmeans_seed(cuda(X), 33, 4, 5, [0.3, 0.75, 0.5])[1].cpu().tolist() == chosen.tolist()


def test_bad_arguments_and_workspace_are_refused_and_nothing_is_launched():
    d = dev()
    lib = L.load()
    X = cr.blobs(130, 33)
    n, k, C = 130, 33, 6
    t = cuda(X)
    need = d.rows_kmeans_ws_bytes(n, C, k)
    assert need == lib.emg_rows_kmeans_ws_bytes(n, C, k) > 16 * n
    for bad in ((0, 1, k), (n, 0, k), (n, n + 1, k), (n, C, 0), (-1, C, k), (2 ** 31, C, k)):
        assert lib.emg_rows_kmeans_ws_bytes(*bad) == 0
        with pytest.raises(ValueError):
            d.rows_kmeans_ws_bytes(*bad)
    GUARD = -7
    start = cuda(X[:C])
    centres = start.clone()
    labels = torch.full((n,), GUARD, dtype=torch.int32, device="cuda")
    chosen = torch.full((C,), GUARD, dtype=torch.int32, device="cuda")
    info = torch.full((4,), -7.0, dtype=torch.float64, device="cuda")
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    import ctypes
    u = (ctypes.c_double * (C - 1))(*([0.5] * (C - 1)))
    u_bad = (ctypes.c_double * (C - 1))(*([0.5] * (C - 2) + [1.0]))

    def lloyd(n=n, ld=k, k=k, ld_c=k, C=C, max_iter=5, tol=0.0, ws_ptr=ws.data_ptr(), ws_bytes=need, X_ptr=t.data_ptr(),
              info_ptr=info.data_ptr()):
        return lib.emg_rows_kmeans(X_ptr, n, ld, k, centres.data_ptr(), ld_c, C, max_iter, tol, labels.data_ptr(), info_ptr,
                                   ws_ptr, ws_bytes, None)

    def seeding(n=n, C=C, first=0, u=u, ws_bytes=need, ws_ptr=ws.data_ptr()):
        return lib.emg_rows_kmeans_seed(t.data_ptr(), n, k, k, C, first, u, centres.data_ptr(), k, chosen.data_ptr(), ws_ptr,
                                        ws_bytes, None)

    for rc in (lloyd(ws_bytes=need - 1), lloyd(ws_bytes=0), lloyd(ws_ptr=ws.data_ptr() + 4), lloyd(ws_ptr=None), lloyd(n=0),
               lloyd(C=0), lloyd(C=n + 1), lloyd(k=0), lloyd(ld=k - 1), lloyd(ld_c=k - 1), lloyd(max_iter=-1), lloyd(tol=-1.0),
               lloyd(tol=float("nan")), lloyd(tol=float("inf")), lloyd(X_ptr=None), lloyd(info_ptr=None),
               lloyd(info_ptr=info.data_ptr() + 4),
               seeding(ws_bytes=need - 1), seeding(ws_ptr=ws.data_ptr() + 8), seeding(first=-1), seeding(first=n), seeding(u=u_bad),
               seeding(u=None), seeding(C=n + 1), seeding(n=0)):
        assert rc != 0
    with pytest.raises(L.EmgError, match="workspace"):
        d.rows_kmeans(t, k, centres, 5, 0.0, ws=ws[:need - 16])
    with pytest.raises(L.EmgError, match="workspace"):
        d.rows_kmeans_seed(t, k, C, 0, [0.5] * (C - 1), ws=ws[:need - 16])
    torch.cuda.synchronize()
    assert (labels == GUARD).all() and (chosen == GUARD).all() and (info == -7.0).all() and (ws == 0).all()
    assert torch.equal(centres, start)
    assert lloyd() == 0 and seeding(C=1, u=None) == 0          # and the same buffers do when the arguments are right
    torch.cuda.synchronize()
    assert (labels >= 0).all() and chosen[0].item() == 0


# ---- the public path ----------------------------------------------------------------------------------
def crafted(cls, ent, rel, k):
    """a fitted model whose parameters are the given arrays"""
    m = cls(k=k, epochs=1, batches_count=1)
    m.ent_to_idx = {"e%03d" % i: i for i in range(len(ent))}
    m.rel_to_idx = {"r%02d" % i: i for i in range(len(rel))}
    m.trained_model_params = [np.ascontiguousarray(ent, F32), np.ascontiguousarray(rel, F32)]
    m.is_fitted = True
    return m


class Recorder:
    def fit_predict(self, emb):
        self.emb = emb
        return list(range(len(emb)))[::-1]


@pytest.mark.parametrize("cls,width", [(DistMult, 1), (ComplEx, 2)])
def test_find_clusters_with_the_estimator_in_three_modes(cls, width):
    k = 6
    ent = cr.blobs(130, width * k)
    rel = cr.normal(9, width * k, scale=0.3)
    m = crafted(cls, ent, rel, k)
    E = np.array(["e%03d" % i for i in range(130)])
    for kw in (dict(init="k-means++", seed=3), dict(init="random", n_init=4, seed=1), dict(init=ent[[5, 50, 100, 120]])):
        C = 4
        got = discovery.find_clusters(E, m, discovery.KMeans(C, max_iter=50, **kw), mode="entity")
        want, inertias = R.kmeans(ent, C, init=kw["init"], n_init=kw.get("n_init", "auto"), max_iter=50, seed_value=kw.get("seed", 0))
        assert got.dtype == np.int32 and np.array_equal(got, want["labels"]), kw
    km = discovery.KMeans(4, init="random", n_init=4, seed=1, max_iter=50)
    km.fit(cuda(ent))
    want, inertias = R.kmeans(ent, 4, init="random", n_init=4, max_iter=50, seed_value=1)
    assert km.n_restarts_ == 4 and km.n_iter_ == want["n_iter"] and len(set(inertias)) > 1 and want["restart"] == int(np.argmin(inertias))
    assert np.array_equal(bits(km.cluster_centers_), bits(want["centres"]))
    assert abs(km.inertia_ - want["inertia"]) <= 130 * 2.0 ** -52 * want["inertia"]
    # a selection in another order with a repeated label: rows are not de-duplicated
    sel = [7, 3, 7, 129, 64, 1, 0, 99]
    got = discovery.find_clusters(E[sel], m, discovery.KMeans(3, seed=2), "entity")
    assert np.array_equal(got, R.kmeans(ent[sel], 3, seed_value=2)[0]["labels"])
    R_ = np.array(["r%02d" % i for i in range(9)])
    got = discovery.find_clusters(R_, m, discovery.KMeans(2, seed=4), mode="relation")
    assert np.array_equal(got, R.kmeans(rel, 2, seed_value=4)[0]["labels"])
    rng = np.random.default_rng(8)
    ids = np.stack([rng.integers(0, 130, 70), rng.integers(0, 9, 70), rng.integers(0, 130, 70)], axis=1)
    T = np.array([["e%03d" % s, "r%02d" % p, "e%03d" % o] for s, p, o in ids])
    rows = np.concatenate([ent[ids[:, 0]], rel[ids[:, 1]], ent[ids[:, 2]]], axis=1)
    assert rows.shape == (70, 3 * width * k)
    got = discovery.find_clusters(T, m, discovery.KMeans(5, seed=6), mode="triple")
    assert np.array_equal(got, R.kmeans(rows, 5, seed_value=6)[0]["labels"])
    with pytest.raises(ValueError, match="n_clusters"):
        discovery.find_clusters(E[:3], m, discovery.KMeans(4))
    # any other object still gets a host array
    rec = Recorder()
    got = discovery.find_clusters(E[sel], m, rec)
    assert isinstance(got, np.ndarray) and got.tolist() == list(range(8))[::-1]
    assert isinstance(rec.emb, np.ndarray) and rec.emb.dtype == F32 and np.array_equal(rec.emb, ent[sel])


def test_labels_equal_scikit_learn_on_separated_tables():
    sk = pytest.importorskip("sklearn.cluster")
    for n, k, C in cases.SEPARATED:
        X, first = cases.separated(n, k, C)
        km = discovery.KMeans(C, init=X[first], max_iter=100, tol=0.0).fit(X)
        fit = sk.KMeans(C, init=X[first], n_init=1, algorithm="lloyd", tol=0, max_iter=100).fit(X)
        assert np.array_equal(km.labels_, fit.labels_), (n, k, C)
