"""discovery.KMeans / emg_rows_kmeans, host side (no GPU): the declared interface, argument validation (every check runs before
the device is asked for), the reference tests/_kmeans_ref.py on hand-sized sets, its agreement with scikit-learn on the
separated tables, and that the cases of tests/test_kmeans.py have the structure each is there for."""
import os
import re

import numpy as np
import pytest

import emgraph_amd
from emgraph_amd import _lib as L
from emgraph_amd.discovery import KMeans, find_clusters
from emgraph_amd.models import ComplEx
from tests import _chain_ref as cr
from tests import _kmeans_cases as cases
from tests import _kmeans_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _n_args(hdr, res, name):
    decl = re.search(r"\b%s\s+%s\s*\(([^;]*)\)\s*;" % (res, name), hdr)
    assert decl, "%s is not declared" % name
    return len(decl.group(1).split(","))


def test_header_and_signatures_declare_kmeans():
    with open(os.path.join(ROOT, "include", "emgraph_hip.h")) as f:
        hdr = f.read()
    assert _n_args(hdr, "size_t", "emg_rows_kmeans_ws_bytes") == 3 == len(L.SIGNATURES["emg_rows_kmeans_ws_bytes"][1])
    assert _n_args(hdr, "int", "emg_rows_kmeans") == 14 == len(L.SIGNATURES["emg_rows_kmeans"][1])
    assert _n_args(hdr, "int", "emg_rows_kmeans_seed") == 13 == len(L.SIGNATURES["emg_rows_kmeans_seed"][1])
    assert re.search(r"#define\s+EMG_ABI_VERSION\s+9\b", hdr) and L.ABI_VERSION == 9
    assert "KEEPS its centre" in hdr and "D^2 sampling" in hdr
    assert emgraph_amd.discovery.KMeans is KMeans
    with open(os.path.join(ROOT, "emgraph_amd", "csrc", "build.sh")) as f:
        assert re.search(r"\bemg_kmeans\b", f.read())


def _fitted_stub():
    m = ComplEx(k=4, epochs=1, batches_count=1)
    m.ent_to_idx = {"a": 0, "b": 1, "c": 2}
    m.rel_to_idx = {"r": 0, "q": 1}
    m.is_fitted = True
    return m


def test_constructor_validation():
    km = KMeans()
    assert (km.n_clusters, km.init, km.n_init, km.max_iter, km.tol, km.seed) == (8, "k-means++", "auto", 300, 1e-4, 0)
    assert KMeans(init="random")._restarts() == 10 and KMeans()._restarts() == 1 and KMeans(n_init=50)._restarts() == 50
    assert KMeans(2, init=np.zeros((2, 3)))._restarts() == 1 and KMeans(2, init=[[0, 1], [2, 3]]).init.dtype == F32
    for bad in (0, -1, 2.0, "8", None, True):
        with pytest.raises(ValueError, match="n_clusters"):
            KMeans(bad)
    for bad in ("kmeans++", None, 3, np.zeros(3), np.zeros((3, 2)), np.zeros((2, 0)), [["a", "b"], ["c", "d"]], True):
        with pytest.raises(ValueError, match="init"):
            KMeans(2, init=bad)
    for bad in (0, -2, 1.0, "ten", None, True):
        with pytest.raises(ValueError, match="n_init"):
            KMeans(n_init=bad)
    for bad in (0, -1, 10.0, "300", None, True):
        with pytest.raises(ValueError, match="max_iter"):
            KMeans(max_iter=bad)
    for bad in (-1e-4, float("nan"), float("inf"), "1e-4", None, True):
        with pytest.raises(ValueError, match="tol"):
            KMeans(tol=bad)
    for bad in (-1, 1.0, "0", None, True):
        with pytest.raises(ValueError, match="seed"):
            KMeans(seed=bad)


def test_fit_and_find_clusters_validation_runs_before_the_device_is_needed():
    X = np.zeros((5, 3), F32)
    for bad in (np.zeros(5, F32), np.zeros((5, 3), np.float64), np.zeros((5, 3, 1), F32), np.zeros((5, 0), F32), [["a"]]):
        with pytest.raises(ValueError, match="rows"):
            KMeans(2).fit(bad)
    with pytest.raises(ValueError, match="n_clusters"):
        KMeans(6).fit(X)
    with pytest.raises(ValueError, match="n_clusters"):
        KMeans(6).fit_predict(X)
    with pytest.raises(ValueError, match="columns"):
        KMeans(2, init=np.zeros((2, 4))).fit(X)
    with pytest.raises(RuntimeError, match="not fitted"):
        KMeans(2).predict(X)
    fitted = KMeans(2)
    fitted.cluster_centers_ = np.zeros((2, 4), F32)
    with pytest.raises(ValueError, match="columns"):
        fitted.predict(X)
    # find_clusters: the estimator is an object with fit_predict like any other, plus the row count
    m = _fitted_stub()
    E = np.array(["a", "b"])
    with pytest.raises(ValueError, match="n_clusters"):
        find_clusters(E, m, KMeans(3))
    with pytest.raises(ValueError, match="n_clusters"):
        find_clusters(np.array([], dtype=str), m, KMeans(1))
    with pytest.raises(ValueError, match="n_clusters"):
        find_clusters(np.array([["a", "r", "b"]]), m, KMeans(2), mode="triple")
    for kw in ({"eps": 0.3}, {"min_samples": 4}, {"metric": "cosine"}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            find_clusters(E, m, KMeans(2), **kw)
    with pytest.raises(ValueError, match="mode"):
        find_clusters(E, m, KMeans(2), mode="entities")
    with pytest.raises(ValueError, match="entities"):
        find_clusters(np.array(["a", "zzz"]), m, KMeans(2))
    with pytest.raises(RuntimeError, match="not been fitted"):
        find_clusters(E, ComplEx(k=4, epochs=1, batches_count=1), KMeans(2))
    with pytest.raises(ValueError, match="clustering_algorithm"):
        find_clusters(E, m, "kmeans")                       # the string stays refused: the estimator is the way in


def test_reference_on_hand_checked_sets():
    # a row equally near two centres takes the lower index
    X = np.array([[0, 0], [2, 0], [1, 0], [1, 1]], F32)
    labels, dist, margin = R.assign(X, np.array([[2, 0], [0, 0]], F32))
    assert labels.tolist() == [1, 0, 0, 0] and dist.tolist() == [0.0, 0.0, 1.0, np.sqrt(F32(2))] and margin == 0.0
    run = R.lloyd(X, np.array([[2, 0], [0, 0]], F32), 10, 0.0)
    assert run["labels"].tolist() == [1, 0, 0, 0] and run["centres"].tolist() == [[F32(4) / F32(3), F32(1) / F32(3)], [0, 0]]
    assert run["n_iter"] == 1 and run["converged"] and run["stopped_by"] == "labels"
    assert abs(run["inertia"] - 12 / 9) < 1e-6
    # duplicate start rows: the higher cluster is empty and keeps its centre (which then takes the row lying on it)
    run = R.lloyd(X, np.array([[0, 0], [0, 0]], F32), 1, 0.0)
    assert R.assign(X, np.zeros((2, 2), F32))[0].tolist() == [0, 0, 0, 0] and run["min_count"] == 0
    assert run["centres"].tolist() == [[1.0, 0.25], [0.0, 0.0]] and run["labels"].tolist() == [1, 0, 0, 0]
    # one cluster: the mean, one update, the labels cannot change
    run = R.lloyd(X, X[:1], 10, 1e-4)
    assert run["labels"].tolist() == [0, 0, 0, 0] and run["centres"].tolist() == [[1.0, 0.25]] and run["n_iter"] == 1
    assert run["tol_abs"] == 1e-4 * ((0.5 + 0.1875) / 2)
    # a NaN row: no label, no share in the mean or the inertia
    Xn = np.array([[0, 0], [np.nan, 1], [4, 0]], F32)
    run = R.lloyd(Xn, Xn[:1], 3, 0.0)
    assert run["labels"].tolist() == [0, -1, 0] and run["centres"].tolist() == [[2.0, 0.0]] and run["inertia"] == 8.0
    # the update's order: chunks of 256 members, not one running sum — 1e16 swallows every 1.0 added to it, the second chunk's
    # four ones arrive as 4.0
    rows = np.concatenate([[1e16], np.ones(259)])[:, None]
    sequential = 0.0
    for v in rows[:, 0]:
        sequential += v
    assert sequential == 1e16 and R._chunked_sum(rows)[0] == 1e16 + 4.0
    # the pick: first i with S_i > u S_n, floor(u n) when every weight is 0
    w = np.array([0.0, 1.0, 0.0, 3.0])
    assert [R.pick(w, u)[0] for u in (0.0, 0.2, 0.25, 0.3, 0.999)] == [1, 1, 3, 3, 3]
    assert [R.pick(np.zeros(10), u)[0] for u in (0.0, 0.55, 0.999)] == [0, 5, 9]
    assert R.pick(w, 0.125)[1] == 0.125


def test_reference_equals_sklearn_on_separated_tables():
    """claimed only where no cluster goes empty and every assignment margin exceeds the stated separation — and every listed
    table must qualify"""
    sk = pytest.importorskip("sklearn.cluster")
    claimed = 0
    for n, k, C in cases.SEPARATED:
        X, first = cases.separated(n, k, C)
        run = R.lloyd(X, X[first], 100, 0.0)
        if run["min_count"] == 0 or not run["assign_margin"] > cases.SEPARATION:
            continue
        claimed += 1
        fit = sk.KMeans(C, init=X[first], n_init=1, algorithm="lloyd", tol=0, max_iter=100).fit(X)
        assert np.array_equal(fit.labels_, run["labels"]), (n, k, C)
        assert run["converged"] and np.bincount(run["labels"], minlength=C).min() >= 1
    assert claimed == len(cases.SEPARATED)


def test_no_case_is_vacuous():
    ns, ks, Cs = (set(s[i] for s in cases.SHAPES) for i in range(3))
    assert ns == {1, 2, 63, 64, 65, 130, 257, 1000} and ks == {1, 3, 31, 32, 33, 40, 100} and Cs == {1, 2, 6, 63, 64, 65, 130}
    ties = empties = multi = 0
    for n, k, C in cases.SHAPES:
        assert C <= n
        for name, X in cases.tables(n, k).items():
            run = R.lloyd(X, X[cases.start_rows(n, C)], cases.MAX_ITER, 0.0)
            assert run["stopped_by"] == "labels", (name, n, k, C)       # MAX_ITER is enough everywhere
            ties += run["assign_margin"] == 0.0
            empties += run["min_count"] == 0
            multi += run["n_iter"] >= 5
    assert ties >= 10 and empties >= 10 and multi >= 10
    for name, sizes in cases.SIZED.items():
        X, start, owner = cases.sized_clusters(sizes)
        assert np.array_equal(R.assign(X, start)[0], owner) and len(X) > 3 * 256
        blocks = {(c, b) for c, b in zip(owner.tolist(), (np.arange(len(owner)) // 256).tolist())}
        assert all((c, b) in blocks for c in range(3) for b in range(3))            # members in every block of the sort
    assert 255 in cases.SIZED["around_the_chunk"] and 256 in cases.SIZED["around_the_chunk"] and 257 in cases.SIZED["around_the_chunk"]
    assert max(cases.SIZED["one_holds_most"]) > 3 * 256
    X, start, tol = cases.tol_case()
    run = R.lloyd(X, start, 100, tol)
    assert run["stopped_by"] == "tol" and run["stop_margin"] > 1e-3 and run["near_tol"] > 1e-3 and run["n_iter"] > 3
    assert R.lloyd(X, start, 100, 0.0)["n_iter"] > run["n_iter"]                     # the tolerance is what stopped it
    # seeding: every pick is decided by far more than the rounding of an f64 prefix sum (n 2^-53 = 1e-13 at n = 1000)
    for maker, n, k, C, seed in cases.SEED_CASES:
        X = cases.integers(n, k) if maker == "integers" else cr.MAKERS[maker](n, k)
        picks = set()
        for restart in range(3):
            first, u = R.draws(seed, restart, n, C, "k-means++")
            chosen, centres, margin = R.seed(X, C, first, u)
            assert margin > 1e-9, (maker, n, C, restart, margin)
            assert np.array_equal(centres, X[chosen]) and chosen[0] == first
            picks.add(tuple(chosen.tolist()))
        assert len(picks) == 3 or n <= 2
    # the restarts of the public-path test do not all end alike
    ent = cr.blobs(130, 6)
    best, inertias = R.kmeans(ent, 4, init="random", n_init=4, max_iter=50, seed_value=1)
    assert len(set(inertias)) > 1 and best["restart"] == int(np.argmin(inertias))
    ent = cr.blobs(130, 12)
    best, inertias = R.kmeans(ent, 4, init="random", n_init=4, max_iter=50, seed_value=1)
    assert len(set(inertias)) > 1
