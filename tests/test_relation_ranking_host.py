"""Relation prediction, host side (no GPU): the relation side of the FilterIndex against brute force, the rank assembly on
hand-made counters, the declared interface, and the argument validation of the public functions (every check runs before the
device is asked for)."""
import os
import re

import numpy as np
import pytest

from emgraph_amd import _lib as L
from emgraph_amd.evaluation import (FilterIndex, evaluate_relation_prediction, ranks_from_counts, topn_completions,
                                    topn_relations)
from emgraph_amd.evaluation.ranking import rank_relations_device, topn_relations_device
from emgraph_amd.models import ComplEx
from tests import _relrank_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"emg_eval_rel_rotate_image": 7, "emg_eval_rel_count": 22, "emg_eval_rel_scores_dense": 16, "emg_eval_rel_topn": 11}


def test_header_and_signatures_declare_the_relation_side():
    with open(os.path.join(ROOT, "include", "emgraph_hip.h")) as f:
        hdr = f.read()
    assert re.search(r"#define\s+EMG_ABI_VERSION\s+9\b", hdr) and L.ABI_VERSION == 9
    for sym, n_args in NEW_SYMBOLS.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % sym, hdr)
        assert m, sym
        assert len(m.group(1).split(",")) == n_args == len(L.SIGNATURES[sym][1]), sym
        comment = hdr[:m.start()]
        assert "EmbeddingModel.py:1856-1866" in comment[comment.rindex("/*"):], sym   # the scoring each one extends
    with open(os.path.join(ROOT, "emgraph_amd", "csrc", "build.sh")) as f:
        assert re.search(r"\bemg_relrank\b", f.read())
    if os.path.exists(L.LIB_PATH):
        lib = L.load()
        for sym in NEW_SYMBOLS:
            assert hasattr(lib, sym), sym


# entities 0..9, relations 0..4; (0, 1, 2) twice; the pair (3, 4) holds every relation; relation 7 is unknown to a model of 5
F = np.array([[0, 1, 2], [0, 3, 2], [0, 1, 2], [2, 0, 0], [0, 1, 3], [5, 4, 5], [0, 7, 2]] + [[3, p, 4] for p in range(5)], np.int64)
N_REL = 5


def brute_known(s, o, subset=None):
    known = sorted({int(p) for a, p, b in F if a == s and b == o and p < N_REL and (subset is None or p in subset)})
    return known


def rows_of(ptr, idx):
    assert ptr.dtype == np.int64 and idx.dtype == np.int32 and ptr[0] == 0 and ptr[-1] == len(idx)
    return [idx[ptr[r]:ptr[r + 1]].tolist() for r in range(len(ptr) - 1)]


@pytest.mark.parametrize("subset", [None, [1, 4], [0, 2]])
def test_rel_csr_against_brute_force(subset):
    fi = FilterIndex(F)
    T = np.array([[0, 1, 2], [0, 2, 2], [2, 0, 0], [3, 4, 4], [9, 3, 9], [2, 4, 0], [0, 0, 11], [-1, 2, 0]], np.int64)   # 9, 11, -1: unseen
    got = rows_of(*fi.rel_csr(T, N_REL, subset))
    for (s, p, o), row in zip(T, got):
        want = sorted(set(brute_known(s, o, subset)) | {int(p)})   # p itself is always in its row
        assert row == want, ((s, p, o), row, want)
        assert row == sorted(set(row))                             # ascending, distinct (the duplicated triple once)
    pairs = T[:, [0, 2]]
    got = rows_of(*fi.known_rel_csr(pairs, N_REL, subset))
    for (s, o), row in zip(pairs, got):
        assert row == brute_known(s, o, subset), ((s, o), row)
    assert rows_of(*fi.known_rel_csr(np.zeros((0, 2), np.int64), N_REL)) == []
    with pytest.raises(ValueError):
        fi.rel_csr(np.array([[0, 5, 2]]), N_REL)


def test_rel_csr_leaves_the_entity_sides_alone():
    fi = FilterIndex(F)
    before = [a.copy() for a in fi.csr(F[:3], L.EVAL_S_O, 12)]
    fi.rel_csr(F[:3, :], 8)
    after = fi.csr(F[:3], L.EVAL_S_O, 12)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    empty = FilterIndex(np.zeros((0, 3), np.int64))
    assert rows_of(*empty.rel_csr(np.array([[1, 2, 3]]), N_REL)) == [[2]]
    assert rows_of(*empty.known_rel_csr(np.array([[1, 3]]), N_REL)) == [[]]


def test_rank_assembly_on_hand_made_counters():
    gt, eq, fgt, feq = np.array([3, 0, 2]), np.array([2, 1, 3]), np.array([1, 0, 0]), np.array([1, 1, 2])
    want = {"worst": [4, 1, 4], "best": [3, 1, 3], "middle": [3, 1, 4]}
    for strategy, w in want.items():
        got = ranks_from_counts(gt, eq, fgt, feq, 3, "o", strategy)
        assert got.dtype == np.int64 and got.tolist() == w, strategy
        assert ref.ranks(gt, eq, fgt, feq, strategy).tolist() == w
    # middle: gt + ceil(eq / 2)
    assert ranks_from_counts([0], [3], [0], [1], 1, "o", "middle").tolist() == [2]


def _fitted_stub():
    m = ComplEx(k=4, epochs=1, batches_count=1)
    m.ent_to_idx = {"a": 0, "b": 1, "c": 2}
    m.rel_to_idx = {"r": 0, "q": 1}
    m.is_fitted = True
    return m


def test_validation_runs_before_the_device_is_needed():
    m = _fitted_stub()
    P = np.array([["a", "b"]])
    for bad in (0, L.TOPN_MAX + 1, 2.5, True):
        with pytest.raises(ValueError, match=str(L.TOPN_MAX)):
            topn_relations(P, m, top_n=bad)
        with pytest.raises(ValueError, match=str(L.TOPN_MAX)):
            m.get_topn_relations_idx(np.array([[0, 1]]), top_n=bad)
        with pytest.raises(ValueError, match=str(L.TOPN_MAX)):
            topn_relations_device(L.COMPLEX, None, None, 8, 1.0, np.array([[0, 1]]), bad)
    with pytest.raises(ValueError):
        topn_relations(np.array([["a", "r", "b"]]), m)
    with pytest.raises(ValueError):
        m.get_topn_relations_idx(np.array([[0, 0, 1]]))
    with pytest.raises(ValueError):
        evaluate_relation_prediction(np.array([["a", "b"]]), m)
    with pytest.raises(ValueError):
        m.get_relation_ranks_idx(np.array([[0, 1]]))
    with pytest.raises(ValueError):
        evaluate_relation_prediction([["a", "r", "b"]], m)          # not an array
    with pytest.raises(AssertionError):
        evaluate_relation_prediction(np.array([["a", "r", "b"]]), m, ranking_strategy="median")
    with pytest.raises(ValueError, match="entities"):
        topn_relations(np.array([["a", "zz"]]), m)
    with pytest.raises(ValueError, match="entities"):
        topn_relations(np.array([[0, 3]]), m, from_idx=True)
    with pytest.raises(ValueError, match="relations"):
        topn_relations(P, m, relations_subset=["nope"])
    with pytest.raises(ValueError, match="relations"):
        topn_relations(np.array([[0, 1]]), m, relations_subset=[2], from_idx=True)
    with pytest.raises(ValueError, match="relations"):
        evaluate_relation_prediction(np.array([["a", "zz", "b"]]), m)
    with pytest.raises(ValueError, match="entities"):
        evaluate_relation_prediction(np.array([["a", "r", "zz"]]), m, filter_unseen=False)
    with pytest.raises(ValueError, match="relations"):
        evaluate_relation_prediction(np.array([["a", "r", "b"]]), m, relations_subset=["nope"])
    unfitted = ComplEx(k=4, epochs=1, batches_count=1)
    for call in (lambda: topn_relations(P, unfitted), lambda: unfitted.get_topn_relations_idx(np.array([[0, 1]])),
                 lambda: evaluate_relation_prediction(np.array([["a", "r", "b"]]), unfitted),
                 lambda: unfitted.get_relation_ranks_idx(np.array([[0, 0, 1]]))):
        with pytest.raises(RuntimeError, match="not been fitted"):
            call()


def test_links_and_sharding_are_refused_as_on_the_entity_sides():
    m = _fitted_stub()
    m.embedding_model_params["non_linearity"] = "tanh"
    with pytest.raises(NotImplementedError, match="rank_through_link"):
        m.get_relation_ranks_idx(np.array([[0, 0, 1]]))
    m = _fitted_stub()
    m.embedding_model_params["sharding"] = "rows"
    with pytest.raises(NotImplementedError, match="one GPU"):
        m.get_relation_ranks_idx(np.array([[0, 0, 1]]))
    with pytest.raises(NotImplementedError, match="one GPU"):
        m.get_topn_relations_idx(np.array([[0, 1]]))
    with pytest.raises(NotImplementedError, match="one GPU"):
        rank_relations_device(L.COMPLEX, None, None, 8, 1.0, np.array([[0, 0, 1]]), shard=(0, 2))
    with pytest.raises(ValueError, match="link"):
        rank_relations_device(L.COMPLEX, None, None, 8, 1.0, np.array([[0, 0, 1]]), link=9)


def test_the_entity_side_functions_keep_refusing_the_predicate_side():
    m = _fitted_stub()
    with pytest.raises(ValueError, match="side"):
        topn_completions(np.array([["a", "b"]]), m, side="p")
    from emgraph_amd.evaluation import protocol
    assert "p" not in protocol._SIDES


def test_mixed_tables_tell_chain_orders_apart():
    """the case tests/test_relation_ranking.py::test_chain_order_on_mixed_tables runs on the device: on these tables the C
    oracle's ComplEx chain (re half, then im half) is restated to the bit by a numpy emulation (fmaf through float64), while
    the same emulation with re and im interleaved misses a large share of the scores"""
    from tests import _chain_ref as chain
    F32 = np.float32
    k, n_rel, rows = 25, 21, 40
    E, R = chain.mixed(100, 2 * k, seed=1) * F32(2.0 ** -6), chain.mixed(n_rel, 2 * k, seed=2) * F32(2.0 ** -6)
    rs = np.random.RandomState(5)
    s, o = rs.randint(0, 100, rows), rs.randint(0, 100, rows)
    S = ref.scores("ComplEx", E, R, 2 * k, 1.0, s, o, np.arange(n_rel))
    assert np.abs(S).max() * 1e5 < 2 ** 31

    def fma(a, b, c):
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)

    one = np.ones((1, n_rel), F32)
    s_r, s_i, o_r, o_i = (a[:, None, :] * one[:, :, None] for a in (E[s][:, :k], E[s][:, k:], E[o][:, :k], E[o][:, k:]))
    p_r, p_i = R[None, :, :k], R[None, :, k:]
    q_r = fma(p_r, s_r, -(p_i * s_i))
    q_i = fma(p_r, s_i, p_i * s_r)

    def run(steps):
        acc = np.zeros((rows, n_rel), F32)
        for q, e, j in steps:
            acc = fma(q[:, :, j], e[:, :, j], acc)
        return acc.view(np.int32)

    halves = [(q_r, o_r, j) for j in range(k)] + [(q_i, o_i, j) for j in range(k)]
    mixed_up = [st for j in range(k) for st in ((q_r, o_r, j), (q_i, o_i, j))]
    assert np.array_equal(run(halves), S.view(np.int32))
    assert (run(mixed_up) != S.view(np.int32)).mean() > 0.25
