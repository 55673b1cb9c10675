"""SimplE without a device: the registration, the header's contract, the host references of tests/_simple_ref.py (the float64 gradients
against finite differences, the swap form against the two sums, the float32 chain against float64) and the refusals, which come
before the device is asked for."""
import os
import re

import numpy as np
import pytest

from tests import _simple_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_simple_is_registered():
    from emgraph_amd import _lib as L
    from emgraph_amd import models
    from emgraph_amd.models import MODEL_REGISTRY, ComplEx, SimplE
    assert MODEL_REGISTRY["SimplE"] is SimplE and SimplE.name == "SimplE" and "SimplE" in models.__all__
    assert L.SIMPLE == 8 and L.ROTATE == 6
    m = SimplE(k=7)
    assert m._model_id() == L.SIMPLE and m.internal_k == 14 and m._scale() == 0.5
    assert issubclass(SimplE, ComplEx)


def test_header_defines_the_model_id_and_leaves_7_unassigned():
    text = open(os.path.join(ROOT, "include", "emgraph_hip.h")).read()
    assert re.search(r"^#define EMG_SIMPLE 8$", text, re.M)
    assert re.search(r"^#define EMG_ABI_VERSION 9$", text, re.M)
    names = "TRANSE_L1|TRANSE_L2|DISTMULT|COMPLEX|HOLE|TRANSE_P|ROTATE|SIMPLE"
    ids = {name: int(v) for name, v in re.findall(r"^#define (EMG_(?:%s)) (\d+)$" % names, text, re.M)}
    assert sorted(ids.values()) == [0, 1, 2, 3, 4, 5, 6, 8]          # 7 names no model
    # no define of the block of model ids (from the first id to the corruption sides) has the value 7
    block = text[text.index("#define EMG_TRANSE_L1"):text.index("#define EMG_SIDE_S")]
    assert not re.search(r"^#define \w+ 7$", block, re.M)
    assert "unassigned" in block
    from emgraph_amd import _lib as L
    assert L.ABI_VERSION == 9


def _case(seed=3, n_ent=12, n_rel=3, k=5, n=20):
    rs = np.random.RandomState(seed)
    E = rs.uniform(-0.5, 0.5, (n_ent, 2 * k))
    R = rs.uniform(-0.5, 0.5, (n_rel, 2 * k))
    X = np.stack([rs.randint(0, n_ent, n), rs.randint(0, n_rel, n), rs.randint(0, n_ent, n)], 1)
    X[0, 2] = X[0, 0]                                                 # a triple with s == o
    g = rs.randn(len(X))
    return E, R, X, g, k


def test_float64_gradients_agree_with_finite_differences():
    """central differences, step 1e-6 (the score is trilinear: the truncation term vanishes but for s == o, where it is h^2 times a
    coefficient of order one; rounding ~ eps |L| / h ~ 1e-10) — rtol 1e-6, atol 1e-9 for entries that are zero"""
    E, R, X, g, k = _case()
    assert X[0, 0] == X[0, 2]
    dE, dR = ref.grads_f64(E, R, X, g)
    loss = lambda E_, R_: float(np.dot(g, ref.score_f64(E_, R_, X)))   # noqa: E731
    h = 1e-6
    for T, dT, which in ((E, dE, 0), (R, dR, 1)):
        fd = np.zeros_like(T)
        for idx in np.ndindex(*T.shape):
            tp, tm = T.copy(), T.copy()
            tp[idx] += h
            tm[idx] -= h
            fd[idx] = (loss(tp, R) - loss(tm, R)) / (2 * h) if which == 0 else (loss(E, tp) - loss(E, tm)) / (2 * h)
        np.testing.assert_allclose(dT, fd, rtol=1e-6, atol=1e-9)
    assert np.abs(dR[:, k:]).max() > 0 and np.abs(dR[:, :k]).max() > 0


def test_swap_form_equals_the_two_sums():
    E, R, X, g, k = _case()
    np.testing.assert_allclose(ref.score_f64(E, R, X), ref.score_two_sums_f64(E, R, X), rtol=1e-14, atol=1e-17)
    np.testing.assert_array_equal(ref.swap(ref.swap(E)), E)


def test_float32_chain_on_the_float32_queries_agrees_with_float64():
    """within ref.score_bound: (2k + 3) 2^-24 scale sum |terms| (the query's product is one of the term's roundings)"""
    rs = np.random.RandomState(5)
    for k in (1, 5, 37):
        E = rs.uniform(-0.5, 0.5, (40, 2 * k)).astype(np.float32)
        R = rs.uniform(-0.5, 0.5, (3, 2 * k)).astype(np.float32)
        X = np.stack([rs.randint(0, 40, 30), rs.randint(0, 3, 30), rs.randint(0, 40, 30)], 1)
        want, bound = ref.score_f64(E, R, X), ref.score_bound(E, R, X)
        for obj in (True, False):
            Q = ref.queries_f32(E, R, X, obj)
            np.testing.assert_allclose(Q, ref.queries_f64(E, R, X, obj), rtol=2.0 ** -23)
            S = ref.chain_f32(Q, E)
            assert S.dtype == np.float32 and S.shape == (30, 40)
            got = S[np.arange(len(X)), X[:, 2] if obj else X[:, 0]].astype(np.float64)
            assert np.all(np.abs(got - want) <= bound), (k, obj, np.abs(got - want).max(), bound.min())
    assert ref.cmp_int(np.float32(-1.234567)) == -123456


def test_an_asymmetric_pair_scores_differently():
    E, R, X, g, k = _case()
    a, b = 1, 2
    f_ab = ref.score_f64(E, R, np.array([[a, 0, b]]))[0]
    f_ba = ref.score_f64(E, R, np.array([[b, 0, a]]))[0]
    assert f_ab != f_ba and abs(f_ab - f_ba) > 1e-6


def _fitted(**emp):
    from emgraph_amd.models import SimplE
    m = SimplE(k=4, embedding_model_params=emp)
    m.is_fitted = True
    m.ent_to_idx = {"e%d" % i: i for i in range(6)}
    m.rel_to_idx = {"r0": 0}
    m.trained_model_params = [np.zeros((6, 8), np.float32), np.zeros((1, 8), np.float32)]
    return m


X_LABELS = np.array([["e0", "r0", "e1"], ["e1", "r0", "e2"], ["e2", "r0", "e3"]])


@pytest.mark.parametrize("emp", [{"sharding": "k"}, {"sharding": "batch"}, {"sharding": "range"}, {"shared_negatives": 8}])
def test_fit_refuses_what_simple_has_no_kernel_for(emp):
    from emgraph_amd.models import SimplE
    with pytest.raises(NotImplementedError, match="SimplE"):
        SimplE(k=4, embedding_model_params=emp).fit(X_LABELS)


def test_ranking_refuses_sharding():
    from emgraph_amd import _lib as L
    from emgraph_amd.evaluation.ranking import rank_triples_device
    with pytest.raises(NotImplementedError, match="SimplE"):
        _fitted(sharding="batch").get_ranks_idx(np.array([[0, 0, 1]]))
    z = np.zeros((6, 8), np.float32)
    with pytest.raises(NotImplementedError, match="SimplE"):
        rank_triples_device(L.SIMPLE, z, z[:1], 8, 0.5, np.array([[0, 0, 1]]), "s,o", "worst", shard=(0, 2))


def test_trainer_refuses_sharding():
    from emgraph_amd import _lib as L
    from emgraph_amd.training import Trainer
    z = np.zeros((6, 8), np.float32)
    for sharded in ("k", "batch"):
        with pytest.raises(NotImplementedError, match="SimplE"):
            Trainer(L.SIMPLE, 8, 0.5, z, z[:1], 2, sharded=sharded)


def test_predict_sharded_and_calibrate_with_corruptions_are_refused():
    m = _fitted()
    with pytest.raises(NotImplementedError, match="SimplE"):
        m.predict(X_LABELS, sharded=True)
    with pytest.raises(NotImplementedError, match="SimplE"):
        m.calibrate(X_LABELS, positive_base_rate=0.5)


def test_embeddings_are_the_whole_row():
    m = _fitted()
    m.trained_model_params[1][0] = np.arange(8)
    np.testing.assert_array_equal(m.get_embeddings(["r0"], "relation"), np.arange(8, dtype=np.float32)[None])
    assert m.get_embeddings(["e0", "e1"]).shape == (2, 8)


def test_simple_joins_the_contraction_models_of_the_ranking_paths():
    from emgraph_amd import _lib as L
    from emgraph_amd.evaluation import ranking as RK
    assert L.SIMPLE in RK.CONTRACTION_MODELS
    assert RK._acc_scale(L.SIMPLE, 0.5) == 0.5 and RK._acc_scale(L.COMPLEX, 0.5) == 1.0


def test_device_cases_hold_what_the_device_tests_say_of_them():
    for k, eta in ((5, 2), (65, 82)):
        E, R, X, codes, xneg, keep_s, repl = ref.training_case(k, eta)
        assert X[0, 0] == X[0, 2]
        assert xneg[1, 2] == xneg[1, 0] == X[1, 0] and xneg[2, 0] == xneg[2, 2] == X[2, 2]     # a replacement equal to the kept entity
        np.testing.assert_array_equal(codes & 0x7FFFFFFF, repl)
        np.testing.assert_array_equal(codes < 0, keep_s == 1)
