"""discover_facts, host side (no GPU): the declared interface, argument validation (every check runs before the device is asked
for), the strategy weights on hand-made graphs with known values, grid sizes, seeding and zero-weight entities."""
import math
import os
import re

import numpy as np
import pytest

from emgraph_amd import _lib as L
from emgraph_amd.discovery import STRATEGIES, discover_facts, generate_candidates, strategy_weights
from emgraph_amd.evaluation.ranking import grid_ranks_device
from emgraph_amd.models import ComplEx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_args(hdr, name):
    m = re.search(r"\b(?:int|int64_t)\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_header_and_signatures_declare_the_grid_count():
    with open(os.path.join(ROOT, "include", "emgraph_hip.h")) as f:
        hdr = f.read()
    assert re.search(r"int64_t\s+emg_eval_grid_ws_bytes\s*\(", hdr) and re.search(r"\bint\s+emg_eval_grid_count\s*\(", hdr)
    for name in ("emg_eval_grid_ws_bytes", "emg_eval_grid_count"):
        assert _declared_args(hdr, name) == len(L.SIGNATURES[name][1]), name
    assert len(L.SIGNATURES["emg_eval_grid_count"][1]) == 18 and len(L.SIGNATURES["emg_eval_grid_ws_bytes"][1]) == 2
    # each declaration sits under a comment that cites the reference lines it replaces
    for name in ("emg_eval_grid_ws_bytes", "emg_eval_grid_count"):
        before = hdr[:re.search(r"\b(?:int|int64_t)\s+%s\s*\(" % name, hdr).start()]
        comment = before[before.rindex("/*"):]
        assert "EmbeddingModel.py:1856-1866" in comment and "2010-2033" in comment, name
    thr_max = int(re.search(r"#define\s+EMG_GRID_THR_MAX\s+(\d+)", hdr).group(1))
    assert thr_max >= 256 and thr_max == L.GRID_THR_MAX
    assert re.search(r"#define\s+EMG_ABI_VERSION\s+9\b", hdr) and L.ABI_VERSION == 9
    with open(os.path.join(ROOT, "emgraph_amd", "csrc", "build.sh")) as f:
        assert re.search(r"\bemg_grid\b", f.read())


N_ENT, N_REL = 30, 3


def _stub(link=None, fitted=True):
    params = {} if link is None else {"non_linearity": link}
    m = ComplEx(k=4, epochs=1, batches_count=1, embedding_model_params=params)
    if fitted:
        m.ent_to_idx = {"e%02d" % i: i for i in range(N_ENT)}
        m.rel_to_idx = {"r%d" % i: i for i in range(N_REL)}
        m.is_fitted = True
    return m


def _labels(T):
    return np.array([["e%02d" % s, "r%d" % p, "e%02d" % o] for s, p, o in T])


X = _labels([(i, i % N_REL, (i * 7 + 1) % N_ENT) for i in range(N_ENT)])


def test_validation_runs_before_the_device_is_needed():
    m = _stub()
    with pytest.raises(RuntimeError, match="not been fitted"):
        discover_facts(X, _stub(fitted=False))
    with pytest.raises(RuntimeError, match="not been fitted"):
        generate_candidates(X, _stub(fitted=False), "random_uniform", "r0", 100)
    with pytest.raises(ValueError, match="entities"):
        discover_facts(np.array([["zzz", "r0", "e01"]]), m)
    with pytest.raises(ValueError, match="relations"):
        discover_facts(np.array([["e00", "nope", "e01"]]), m)
    with pytest.raises(ValueError, match="relations"):
        discover_facts(X, m, target_rel="nope")
    with pytest.raises(ValueError, match="relations"):
        discover_facts(X, m, target_rel=["r0", "nope"])
    with pytest.raises(ValueError, match="relations"):
        generate_candidates(X, m, "random_uniform", "nope", 100)
    with pytest.raises(ValueError, match="shape"):
        discover_facts(X[:, :2], m)
    for bad in ("nope", None, 3):
        with pytest.raises(ValueError, match="strategy"):
            discover_facts(X, m, strategy=bad)
        with pytest.raises(ValueError, match="strategy"):
            generate_candidates(X, m, bad, "r0", 100)
    with pytest.raises(ValueError, match="cluster_squares"):
        discover_facts(X, m, strategy="cluster_squares")
    with pytest.raises(ValueError, match="cluster_squares"):
        generate_candidates(X, m, "cluster_squares", "r0", 100)
    for bad in (0, -1, 2.5, True, "10", None):
        with pytest.raises(ValueError, match="top_n"):
            discover_facts(X, m, top_n=bad)
    for bad in (0, -5, 0.0, 1.5, 1e-9, True, "100", None):
        with pytest.raises(ValueError, match="max_candidates"):
            discover_facts(X, m, max_candidates=bad)
        with pytest.raises(ValueError, match="max_candidates"):
            generate_candidates(X, m, "random_uniform", "r0", bad)
    for bad in (-1, 1.5, None):
        with pytest.raises(ValueError, match="seed"):
            discover_facts(X, m, seed=bad)
    with pytest.raises(NotImplementedError, match="non_linearity"):
        discover_facts(X, _stub(link="tanh"), top_n=3)
    with pytest.raises(ValueError, match="cluster_triangles"):   # X is a set of chains: no triangle
        discover_facts(_labels([(0, 0, 1), (1, 0, 2), (2, 1, 3)]), m, strategy="cluster_triangles")
    with pytest.raises(ValueError, match="outside"):
        grid_ranks_device(L.COMPLEX, np.zeros((5, 8), np.float32), None, 8, 1.0, 0, [0, 5], [1])


def _triples(edges, rel=0):
    return np.array([(s, rel, o) for s, o in edges], np.int64)


def test_strategy_weights_triangle_with_a_pendant_node():
    # 0 - 1 - 2 - 0 and 2 - 3; (1, 0) repeats an edge in the other direction, (3, 3) is a self-loop, entity 4 is isolated
    T = _triples([(0, 1), (1, 2), (2, 0), (2, 3), (1, 0), (3, 3), (0, 1)])
    assert strategy_weights(T, 5, "random_uniform").tolist() == [1, 1, 1, 1, 1]
    assert strategy_weights(T, 5, "exhaustive").tolist() == [1, 1, 1, 1, 1]
    assert strategy_weights(T, 5, "entity_frequency").tolist() == [4, 4, 3, 3, 0]
    assert strategy_weights(T, 5, "graph_degree").tolist() == [2, 2, 3, 1, 0]
    assert strategy_weights(T, 5, "cluster_triangles").tolist() == [1, 1, 1, 0, 0]
    assert strategy_weights(T, 5, "cluster_coefficient").tolist() == [1.0, 1.0, 1.0 / 3.0, 0.0, 0.0]


def test_strategy_weights_k4_and_path():
    K4 = _triples([(a, b) for a in range(4) for b in range(a + 1, 4)])
    assert strategy_weights(K4, 4, "graph_degree").tolist() == [3, 3, 3, 3]
    assert strategy_weights(K4, 4, "cluster_triangles").tolist() == [3, 3, 3, 3]
    assert strategy_weights(K4, 4, "cluster_coefficient").tolist() == [1, 1, 1, 1]
    path = _triples([(0, 1), (1, 2), (2, 3)])
    assert strategy_weights(path, 4, "graph_degree").tolist() == [1, 2, 2, 1]
    for strategy in ("cluster_triangles", "cluster_coefficient"):
        with pytest.raises(ValueError, match=strategy):
            strategy_weights(path, 4, strategy)
    with pytest.raises(ValueError, match="graph_degree"):
        strategy_weights(_triples([(2, 2)]), 4, "graph_degree")


@pytest.mark.parametrize("max_candidates,n_s,n_o", [(100, 10, 10), (99, 9, 11), (1, 1, 1), (7, 2, 3), (900, 30, 30),
                                                    (10 ** 6, 30, 30), (0.5, 21, 21), (1.0, 30, 30), (0.01, 3, 3)])
def test_grid_sizes(max_candidates, n_s, n_o):
    cells = max_candidates if isinstance(max_candidates, int) else int(max_candidates * N_ENT * N_ENT)
    assert n_s == min(math.isqrt(cells), N_ENT) and n_o == min(cells // n_s, N_ENT)   # the rule, restated
    S, O = generate_candidates(X, _stub(), "random_uniform", "r1", max_candidates, seed=3)
    assert S.dtype == np.int64 and O.dtype == np.int64
    assert (len(S), len(O)) == (n_s, n_o) and len(S) * len(O) <= cells
    for ids in (S, O):   # without replacement, ascending, inside the table
        assert np.array_equal(ids, np.unique(ids)) and ids.min() >= 0 and ids.max() < N_ENT


def test_eligible_entities_bound_the_grid_and_zero_weights_are_never_drawn():
    # a triangle among 30 entities: 3 of them have triangles, 27 have weight zero
    Xt = _labels([(4, 0, 9), (9, 1, 17), (17, 2, 4), (0, 0, 1), (20, 1, 21)])
    m = _stub()
    for seed in range(20):
        S, O = generate_candidates(Xt, m, "cluster_triangles", "r0", 100, seed=seed)
        assert S.tolist() == [4, 9, 17] and O.tolist() == [4, 9, 17]
        S, O = generate_candidates(Xt, m, "cluster_triangles", "r0", 2, seed=seed)
        assert len(S) == 1 and len(O) == 2 and set(S) | set(O) <= {4, 9, 17}
        S, O = generate_candidates(Xt, m, "entity_frequency", "r2", 16, seed=seed)
        assert len(S) == 4 and len(O) == 4 and set(S) | set(O) <= {0, 1, 4, 9, 17, 20, 21}


def test_exhaustive_takes_every_entity_and_ignores_max_candidates():
    for mc in (1, 100, "ignored"):
        S, O = generate_candidates(X, _stub(), "exhaustive", "r2", mc)
        assert np.array_equal(S, np.arange(N_ENT)) and np.array_equal(O, np.arange(N_ENT))


@pytest.mark.parametrize("strategy", [s for s in STRATEGIES if s not in ("exhaustive", "cluster_triangles", "cluster_coefficient")])
def test_seed_and_relation_decide_the_grid(strategy):
    m = _stub()
    a = generate_candidates(X, m, strategy, "r0", 64, seed=5)
    b = generate_candidates(X, m, strategy, "r0", 64, seed=5)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    c = generate_candidates(X, m, strategy, "r1", 64, seed=5)
    d = generate_candidates(X, m, strategy, "r0", 64, seed=6)
    assert not (np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1]))
    assert not (np.array_equal(a[0], d[0]) and np.array_equal(a[1], d[1]))
    # the draw is the documented one
    w = strategy_weights(np.array([[int(s[1:]), int(p[1:]), int(o[1:])] for s, p, o in X]), N_ENT, strategy)
    rng = np.random.default_rng([5, 0])
    S = rng.choice(N_ENT, size=8, replace=False, p=w / w.sum())
    O = rng.choice(N_ENT, size=8, replace=False, p=w / w.sum())
    assert np.array_equal(a[0], np.sort(S)) and np.array_equal(a[1], np.sort(O))
