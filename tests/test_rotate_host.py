"""RotatE without a device: the registration, the header's contract, the host references of tests/_rotate_ref.py (the float64 gradients
against finite differences, the float32 chain against float64) and the refusals, which come before the device is asked for."""
import os
import re

import numpy as np
import pytest

from tests import _rotate_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rotate_is_registered():
    from emgraph_amd import _lib as L
    from emgraph_amd.models import MODEL_REGISTRY, ComplEx, RotatE
    assert MODEL_REGISTRY["RotatE"] is RotatE and RotatE.name == "RotatE"
    assert L.ROTATE == 6 and L.TRANSE_P == 5
    m = RotatE(k=7)
    assert m._model_id() == L.ROTATE and m.internal_k == 14 and m._scale() == 1.0
    assert issubclass(RotatE, ComplEx)


def test_header_defines_the_model_id():
    text = open(os.path.join(ROOT, "include", "emgraph_hip.h")).read()
    assert re.search(r"^#define EMG_ROTATE 6$", text, re.M)
    assert re.search(r"^#define EMG_ABI_VERSION 9$", text, re.M)
    ids = {name: int(v) for name, v in re.findall(r"^#define (EMG_(?:TRANSE_L1|TRANSE_L2|DISTMULT|COMPLEX|HOLE|TRANSE_P|ROTATE)) (\d+)$", text, re.M)}
    assert sorted(ids.values()) == list(range(7))          # 7 names no model
    from emgraph_amd import _lib as L
    assert L.ABI_VERSION == 9


def _case(seed=3, n_ent=12, n_rel=3, k=5, n=20):
    rs = np.random.RandomState(seed)
    E = rs.uniform(-0.5, 0.5, (n_ent, 2 * k))
    R = np.concatenate([rs.uniform(-np.pi, np.pi, (n_rel, k)), np.zeros((n_rel, k))], 1)
    X = np.stack([rs.randint(0, n_ent, n), rs.randint(0, n_rel, n), rs.randint(0, n_ent, n)], 1)
    X = X[X[:, 0] != X[:, 2]]
    g = rs.randn(len(X))
    return E, R, X, g, k


def test_float64_gradients_agree_with_finite_differences():
    """central differences, step 1e-6: truncation ~ h^2 f''' / 6 and rounding ~ eps |L| / h are both ~ 1e-10 against gradients of
    order one — rtol 1e-6 (atol 1e-9 for entries that are zero, e.g. rows no triple touches)"""
    E, R, X, g, k = _case()
    assert ref.moduli_f64(E, R, X).min() >= 1e-3
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
    assert np.all(dR[:, k:] == 0) and np.abs(dR[:, :k]).max() > 0


def test_zero_modulus_has_zero_gradient():
    E, R, X, g, k = _case()
    R[0] = 0.0
    X = np.array([[4, 0, 4]])
    dE, dR = ref.grads_f64(E, R, X, [1.5])
    assert ref.score_f64(E, R, X)[0] == 0 and not dE.any() and not dR.any()


def test_float32_chain_agrees_with_float64():
    E, R, X, g, k = _case()
    for obj in (True, False):
        Q = ref.queries_f64(E, R, X, obj)
        S = ref.chain_f32(Q, E)
        assert S.dtype == np.float32
        got = S[np.arange(len(X)), X[:, 2] if obj else X[:, 0]]
        np.testing.assert_allclose(got, ref.score_f64(E, R, X), rtol=1e-5)
    assert ref.cmp_int(np.float32(-1.234567)) == -123456


def _fitted(**emp):
    from emgraph_amd.models import RotatE
    m = RotatE(k=4, embedding_model_params=emp)
    m.is_fitted = True
    m.ent_to_idx = {"e%d" % i: i for i in range(6)}
    m.rel_to_idx = {"r0": 0}
    m.trained_model_params = [np.zeros((6, 8), np.float32), np.zeros((1, 8), np.float32)]
    return m


X_LABELS = np.array([["e0", "r0", "e1"], ["e1", "r0", "e2"], ["e2", "r0", "e3"]])


@pytest.mark.parametrize("emp", [{"sharding": "k"}, {"sharding": "batch"}, {"eval_precision": 1}, {"eval_precision": 2}, {"eval_precision": "2"}])
def test_fit_refuses_what_rotate_has_no_kernel_for(emp):
    from emgraph_amd.models import RotatE
    with pytest.raises(NotImplementedError, match="RotatE"):
        RotatE(k=4, embedding_model_params=emp).fit(X_LABELS)


@pytest.mark.parametrize("emp", [{"eval_precision": 1}, {"eval_precision": 2}, {"sharding": "batch"}])
def test_ranking_refuses_the_other_precisions_and_sharding(emp):
    with pytest.raises(NotImplementedError, match="RotatE"):
        _fitted(**emp).get_ranks_idx(np.array([[0, 0, 1]]))


def test_predict_sharded_discover_facts_and_calibrate_with_corruptions_are_refused():
    from emgraph_amd.discovery import discover_facts
    m = _fitted()
    with pytest.raises(NotImplementedError, match="RotatE"):
        m.predict(X_LABELS, sharded=True)
    with pytest.raises(NotImplementedError, match="RotatE"):
        discover_facts(X_LABELS, m, top_n=3, max_candidates=9)
    with pytest.raises(NotImplementedError, match="RotatE"):
        m.calibrate(X_LABELS, positive_base_rate=0.5)


def test_relation_embeddings_are_the_phases():
    m = _fitted()
    m.trained_model_params[1][0] = np.arange(8)
    np.testing.assert_array_equal(m.get_embeddings(["r0"], "relation"), np.arange(4, dtype=np.float32)[None])
    assert m.get_embeddings(["e0", "e1"]).shape == (2, 8)


# the wide cases of tests/test_rotate.py (its WIDE and (65, ETA_WIDE)), one by one: other combinations of these widths are not
WIDE_CASES = [(65, 2, np.pi), (65, 5, np.pi), (100, 5, np.pi), (128, 2, np.pi), (200, 2, np.pi), (513, 2, np.pi), (513, 5, np.pi),
              (520, 5, np.pi), (100, 5, 20.0), (128, 2, 20.0), (200, 2, 20.0), (200, 5, 20.0), (640, 2, 20.0), (65, 82, np.pi)]


@pytest.mark.parametrize("phase,eta,k", [(phase, eta, k) for k in (5, 37, 64) for eta in (2, 5) for phase in (np.pi, 20.0)]
                         + [(phase, eta, k) for k, eta, phase in WIDE_CASES])
def test_device_cases_are_well_conditioned(k, eta, phase):
    """the condition tests/test_rotate.py states for its gradient comparison, on the cases it uses: every modulus but the planted
    triple's is >= 1e-3, and the planted triple's are exactly 0"""
    E, R, X, codes, xneg, keep_s, repl = ref.training_case(k, eta, phase)
    assert ref.well_conditioned(E, R, X, xneg)
    assert not ref.moduli_f64(E, R, X[:1]).any()
    assert tuple(X[0]) == (ref.PLANT, 4, ref.PLANT) and X[1:, [0, 2]].max() < 128 and repl.max() < 128 and not R[:, k:].any()
    np.testing.assert_array_equal(codes & 0x7FFFFFFF, repl)
    np.testing.assert_array_equal(codes < 0, keep_s == 1)


def test_backward_dry_run_reports_the_generic_pass_and_the_refusals():
    """emg_train_backward_form with EMG_ROTATE: what it answers for EMG_TRANSE_P — the backward pass and the model, riders alone —
    and the same requirements (external dL/dscore, no in-place form); odd k_int is EMG_EINVAL"""
    from emgraph_amd import _lib as L
    from tests.test_step_forms import ALONE, EINVAL, form, make_args
    a = make_args(fused=False)
    a.model = L.ROTATE
    for riders, flags in ((0, 0), (1, ALONE)):
        rc, err, out = form(a, riders)
        assert rc == 0 and out == [0, 0, 0, 0, flags, 0], (rc, err, out)          # (form() checks the pass and the model)
    for kw in ({}, {"fused": False, "opt": "sgd"}):
        b = make_args(**kw)
        b.model = L.ROTATE
        rc, err, _ = form(b)
        assert rc == EINVAL and "EMG_ROTATE trains through" in err, (rc, err)
    a.k_int = 31
    rc, err, _ = form(a)
    assert rc == EINVAL and "EMG_ROTATE" in err and "even" in err, (rc, err)
