"""find_clusters / emg_rows_dbscan, host side (no GPU): the declared interface, argument validation (every check runs before
the device is asked for), and the reference the GPU test compares with — pinned to scikit-learn's DBSCAN, and checked to
give every case of tests/test_clusters.py the structure that case is there for."""
import os
import re

import numpy as np
import pytest

import emgraph_amd
from emgraph_amd import _lib as L
from emgraph_amd.discovery import find_clusters
from emgraph_amd.models import ComplEx
from tests import _dbscan_cases as cases
from tests._dbscan_ref import dbscan_ref, summary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _n_args(hdr, res, name):
    decl = re.search(r"\b%s\s+%s\s*\(([^;]*)\)\s*;" % (res, name), hdr)
    assert decl, "%s is not declared" % name
    return len(decl.group(1).split(","))


def test_header_and_signatures_declare_dbscan():
    with open(os.path.join(ROOT, "include", "emgraph_hip.h")) as f:
        hdr = f.read()
    assert _n_args(hdr, "size_t", "emg_rows_dbscan_ws_bytes") == 2 == len(L.SIGNATURES["emg_rows_dbscan_ws_bytes"][1])
    assert _n_args(hdr, "int", "emg_rows_dbscan") == 13 == len(L.SIGNATURES["emg_rows_dbscan"][1])
    assert re.search(r"#define\s+EMG_ABI_VERSION\s+9\b", hdr) and L.ABI_VERSION == 9
    assert "sklearn.cluster.DBSCAN" in hdr
    assert emgraph_amd.discovery.find_clusters is find_clusters


def _fitted_stub():
    m = ComplEx(k=4, epochs=1, batches_count=1)
    m.ent_to_idx = {"a": 0, "b": 1, "c": 2}
    m.rel_to_idx = {"r": 0, "q": 1}
    m.is_fitted = True
    return m


class _Clusterer:
    def fit_predict(self, emb):
        raise AssertionError("the rows are on the device: validation must come first")


def test_find_clusters_validation_runs_before_the_device_is_needed():
    m = _fitted_stub()
    X = np.array(["a", "b"])
    with pytest.raises(ValueError, match="mode"):
        find_clusters(X, m, mode="entities")
    with pytest.raises(ValueError, match="metric"):
        find_clusters(X, m, metric="euclidean")
    for bad in ("kmeans", None, 3, object()):
        with pytest.raises(ValueError, match="clustering_algorithm"):
            find_clusters(X, m, clustering_algorithm=bad)
    for bad in (-1.0, float("nan"), float("inf"), None, "0.5", True):
        with pytest.raises(ValueError, match="eps"):
            find_clusters(X, m, eps=bad)
    for bad in (0, -3, 2.0, 2.5, None, "5", True):
        with pytest.raises(ValueError, match="min_samples"):
            find_clusters(X, m, min_samples=bad)
    with pytest.raises(ValueError, match="entities"):
        find_clusters(np.array(["a", "zzz"]), m)
    with pytest.raises(ValueError, match="relations"):
        find_clusters(np.array(["r", "a"]), m, mode="relation")
    with pytest.raises(ValueError, match="shape"):
        find_clusters(np.array([["a", "r", "b"]]), m)
    with pytest.raises(ValueError, match="shape"):
        find_clusters(np.array([["a", "r"], ["b", "r"]]), m, mode="triple")
    with pytest.raises(ValueError, match="entities"):
        find_clusters(np.array([["a", "r", "b"], ["a", "r", "zzz"]]), m, mode="triple")
    with pytest.raises(ValueError, match="relations"):
        find_clusters(np.array([["a", "r", "b"], ["a", "nope", "b"]]), m, mode="triple")
    with pytest.raises(RuntimeError, match="not been fitted"):
        find_clusters(X, ComplEx(k=4, epochs=1, batches_count=1))
    # an object with fit_predict: the three device parameters must be left alone, and the other checks hold as well
    for kw in ({"eps": 0.3}, {"min_samples": 4}, {"metric": "cosine"}, {"eps": 1}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            find_clusters(X, m, _Clusterer(), **kw)
    with pytest.raises(ValueError, match="mode"):
        find_clusters(X, m, _Clusterer(), mode="entities")
    with pytest.raises(ValueError, match="entities"):
        find_clusters(np.array(["a", "zzz"]), m, _Clusterer())
    with pytest.raises(RuntimeError, match="not been fitted"):
        find_clusters(X, ComplEx(k=4, epochs=1, batches_count=1), _Clusterer())
    # nothing to cluster: no device either
    out = find_clusters(np.array([], dtype=str), m)
    assert out.dtype == np.int32 and out.shape == (0,)


def test_reference_on_hand_checked_sets():
    labels, core = dbscan_ref(cases.within_l2(cases.shared_border(), 1.0), 4)
    assert core.tolist() == [True, False, False, False, True, False, False, False]
    assert labels.tolist() == [0, 0, 0, 0, 1, 1, 1, -1]              # row 3 touches both clusters: the lower label
    labels, core = dbscan_ref(cases.within_l2(cases.border_before_core(), 1.0), 4)
    assert np.nonzero(core)[0].tolist() == [1, 5]
    assert labels.tolist() == [1, 0, 0, 0, 0, 1, 1, 1, -1]           # numbered by core rows: row 0 is in cluster 1
    labels, core = dbscan_ref(cases.within_l2(cases.blobs(), 1.0), 5)
    assert summary(labels, core) == (3, 3 * 32, 3 * 4 + 9) and core.sum() == 3 * 64
    assert labels[:3].tolist() == [-1, -1, -1]                       # the grids' first corners


def test_reference_equals_sklearn_on_the_gpu_tests_tables():
    """eps = sqrt(m + 0.5) for the integer m the GPU test's radius stands for: the same pairs are within it (squared distances
    are integers), and none sits on the boundary of scikit-learn's float64 arithmetic"""
    sk = pytest.importorskip("sklearn.cluster")

    def check(table, m, min_samples, where):
        within = cases.distances_l2(table)[1] <= m
        labels, core = dbscan_ref(within, min_samples)
        fit = sk.DBSCAN(eps=float(np.sqrt(m + 0.5)), min_samples=min_samples, metric="euclidean", algorithm="brute")
        got = fit.fit_predict(table.astype(np.float64))
        assert np.array_equal(got, labels), where
        assert np.array_equal(fit.core_sample_indices_, np.nonzero(core)[0]), where

    for n in cases.N_RANDOM:
        for table, k, radii in cases.random_cases(n):
            for m, eps in radii:
                assert np.array_equal(cases.within_l2(table, eps), cases.distances_l2(table)[1] <= m)
                for min_samples in cases.MIN_SAMPLES:
                    check(table, m, min_samples, "n %d k %d m %d min_samples %d" % (n, k, m, min_samples))
    for name, (table, k, eps, min_samples) in cases.crafted_cases().items():
        m = int(round(eps * eps))
        assert float(np.sqrt(np.float32(m))) == eps
        for order in (np.arange(len(table)), cases.permutation(name, len(table))):
            check(table[order], m, min_samples, name)


def test_no_crafted_case_is_vacuous():
    for name, (table, k, eps, min_samples) in cases.crafted_cases().items():
        assert table.shape[1] == k
        results = []
        for order in (np.arange(len(table)), cases.permutation(name, len(table))):
            labels, core = dbscan_ref(cases.within_l2(table[order], eps), min_samples)
            clusters, border, noise = summary(labels, core)
            assert clusters >= 2, name
            assert (border >= 1) == cases.expects_border(min_samples), name
            assert (noise >= 1) == cases.expects_noise(min_samples), name
            results.append((order, labels))
        # the numbering depends on the row order: the permuted result is not the given one carried along
        (o0, l0), (o1, l1) = results
        assert not np.array_equal(l1, l0[o1]), name
    table, k, eps, min_samples = cases.crafted_cases()["blobs"]
    assert len(table) > 256
    labels, _ = dbscan_ref(cases.within_l2(table, eps), min_samples)
    for c in range(3):
        rows = np.nonzero(labels == c)[0]
        assert rows.min() < 64 and rows.max() >= 256, "every cluster spans the A workgroups and B tiles"
    # the random tables: the planted identical rows are cores at eps = 0, and something is noise
    for n in (64, 257, 1000):
        table, k, radii = cases.random_cases(n)[-1]
        labels, core = dbscan_ref(cases.within_l2(table, 0.0), 3)
        assert summary(labels, core)[0] >= 2 and (labels < 0).any()
    # cosine: four clusters and four noise rows, the margin the bundles' docstring states
    X = cases.bundles()
    D = cases.cosine_distances(X)
    assert (np.abs(D - cases.COSINE_EPS) > 0.04).all()
    labels, core = dbscan_ref(D <= cases.COSINE_EPS, cases.COSINE_MIN_SAMPLES)
    assert summary(labels, core) == (4, 0, 4) and labels[:4].tolist() == [0, 1, 2, 3]
