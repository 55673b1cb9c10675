"""FocusE on the host (no GPU): the normalisation / NaN fill of the edge values against a literal transcription of the reference
(EmbeddingModel.py:1181-1228, 1099-1108), the structure-weight schedule (:692-714), the float64 helper's softplus against
values recorded from the reference's own ``custom_softplus`` (tests/golden/focuse.npz), and ABI 9."""
import os
import re

import numpy as np
import pytest

from tests import _focuse_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _fw():
    from emgraph_amd.training import focuse_edge_weights
    return focuse_edge_weights


def _X(rels):
    rels = np.asarray(rels)
    n = len(rels)
    return np.stack([np.arange(n), rels, np.arange(n) + 1], 1)


def test_two_relations_two_columns():
    rs = np.random.RandomState(0)
    X = _X(rs.randint(0, 2, 40))
    v = np.stack([rs.uniform(-3, 8, 40), rs.uniform(10, 20, 40)], 1)
    want = ref.normalize_literal(X, v).mean(1)
    got = _fw()(X[:, 1], v)
    assert got.dtype == np.float32 and got.shape == (40,)
    np.testing.assert_allclose(got, want.astype(np.float32), rtol=0, atol=0)
    # each relation's columns span [0, 1] on their own
    lit = ref.normalize_literal(X, v)
    for r in (0, 1):
        assert lit[X[:, 1] == r].min(0).tolist() == [0.0, 0.0] and lit[X[:, 1] == r].max(0).tolist() == [1.0, 1.0]


def test_constant_relation_becomes_one():
    X = _X([0] * 5 + [1] * 5)
    v = np.array([7.0] * 5 + [1, 2, 3, 4, 5.0])
    got = _fw()(X[:, 1], v)
    np.testing.assert_array_equal(got[:5], np.ones(5, np.float32))
    np.testing.assert_array_equal(got, ref.normalize_literal(X, v).mean(1).astype(np.float32))


def test_values_in_unit_range_left_alone_without_the_flag():
    X = _X([0] * 6)
    v = np.array([0.2, 0.4, 0.9, 0.3, 0.25, 0.8])
    np.testing.assert_array_equal(_fw()(X[:, 1], v, normalize=False), v.astype(np.float32))
    np.testing.assert_array_equal(ref.normalize_literal(X, v, False)[:, 0], v)
    # ... and normalised with it (the default)
    np.testing.assert_array_equal(_fw()(X[:, 1], v), ((v - 0.2) / 0.7).astype(np.float32))


def test_negative_value_is_normalised_despite_the_flag():
    X = _X([0] * 4 + [1] * 4)
    v = np.array([-0.5, 0.0, 0.5, 0.25, 0.1, 0.2, 0.3, 0.4])
    got = _fw()(X[:, 1], v, normalize=False)
    np.testing.assert_array_equal(got, ref.normalize_literal(X, v, False)[:, 0].astype(np.float32))
    np.testing.assert_array_equal(got[:4], np.array([0, 0.5, 1.0, 0.75], np.float32))   # relation 0: min < 0
    np.testing.assert_array_equal(got[4:], v[4:].astype(np.float32))                      # relation 1: left alone
    v2 = np.array([0.5, 1.5, 1.0, 0.75])                                                  # max > 1: the same
    np.testing.assert_array_equal(_fw()(np.zeros(4, int), v2, normalize=False), np.array([0, 1, 0.5, 0.25], np.float32))


def test_all_nan_column_is_drawn():
    X = _X([0] * 8 + [1] * 8)
    rs = np.random.RandomState(1)
    v = np.stack([rs.uniform(0, 5, 16), np.full(16, np.nan)], 1)
    lit = ref.normalize_literal(X, v)
    assert np.isnan(lit[:, 1]).all()                      # the reference leaves such a column as it is ...
    got = _fw()(X[:, 1], v, seed=3)
    fill = 2 * got.astype(np.float64) - lit[:, 0]          # ... and fills it with draws: mean = (col0 + draw) / 2
    assert np.isfinite(got).all() and (fill > -1e-6).all() and (fill < 1 + 1e-6).all()
    assert len(np.unique(np.round(fill, 5))) > 8           # draws, not one constant


def test_scattered_nans_filled_once_per_seed():
    rs = np.random.RandomState(2)
    X = _X(rs.randint(0, 3, 60))
    v = rs.uniform(0, 10, (60, 2))
    holes = rs.rand(60, 2) < 0.2
    v[holes] = np.nan
    v0 = v.copy()
    a, b, c = _fw()(X[:, 1], v, seed=5), _fw()(X[:, 1], v, seed=5), _fw()(X[:, 1], v, seed=6)
    np.testing.assert_array_equal(v, v0)                   # the caller's array is not written to
    np.testing.assert_array_equal(a, b)
    assert not np.array_equal(a, c)
    lit = ref.normalize_literal(X, v)
    full = ~holes.any(1)
    np.testing.assert_array_equal(a[full], lit[full].mean(1).astype(np.float32))
    # a row with one hole: its known column as the reference normalises it, its hole a draw in [0, 1)
    one = holes.sum(1) == 1
    draw = 2 * a[one].astype(np.float64) - np.nansum(lit[one], 1)
    assert (draw > -1e-6).all() and (draw < 1 + 1e-6).all()
    assert (a >= 0).all() and (a <= 1).all()


def test_fill_and_mean_alone():
    """the adapter branch of fit(): no normalisation, unknown values drawn, rows averaged"""
    from emgraph_amd.training import focuse_fill_and_mean
    v = np.array([[5.0, np.nan], [np.nan, -2.0], [1.0, 3.0]])
    a = focuse_fill_and_mean(v, seed=1)
    np.testing.assert_array_equal(a, focuse_fill_and_mean(v, seed=1))
    assert a.dtype == np.float32 and a[2] == 2.0 and 2.5 <= a[0] < 3.0 and -1.0 <= a[1] < -0.5
    assert np.isnan(v[0, 1])


def test_one_dimensional_input_and_length_mismatch():
    X = _X([0, 0, 0, 1, 1])
    v = np.array([1.0, 2, 3, 5, 9])
    np.testing.assert_array_equal(_fw()(X[:, 1], v), _fw()(X[:, 1], v.reshape(-1, 1)))
    np.testing.assert_array_equal(_fw()(X[:, 1], v), np.array([0, 0.5, 1, 0, 1], np.float32))
    with pytest.raises(AssertionError, match="Each triple must have a numeric value"):
        _fw()(X[:, 1], v[:4])


def test_structure_weight_schedule():
    from emgraph_amd.training import focuse_structure_weight as sw
    assert [sw(e, 4) for e in range(1, 6)] == [0.75, 0.5, 0.25, 0.001, 0.001]
    assert [ref.structure_weight(e, 4) for e in range(1, 6)] == [0.75, 0.5, 0.25, 0.001, 0.001]
    assert sw(1) == 1 - 1 / 251                             # stop_epoch defaults to 251
    assert sw(7, 0) == 0.001 and sw(7, 0, 0.3) == 0.3 and sw(1, 0, 1.0) == 1.0 and sw(1, 0, 0.0) == 0.0
    for bad in (-0.1, 1.5):
        with pytest.raises(AssertionError, match="Invalid structure_weight"):
            sw(1, 0, bad)
    with pytest.raises(AssertionError, match="Invalid value for stop_epoch"):
        sw(1, -1)


def test_helper_softplus_is_the_references():
    g = np.load(os.path.join(HERE, "golden", "focuse.npz"))
    val, grad = ref.custom_softplus(g["x"])
    np.testing.assert_allclose(val, g["value_f64"], rtol=1e-14, atol=0)
    np.testing.assert_allclose(grad, g["grad_f64"], rtol=1e-14, atol=0)
    y, dy = ref.link("softplus", g["x"])
    np.testing.assert_array_equal(y, val)
    np.testing.assert_array_equal(dy, grad)
    # what pins the constant: at x = -log(9999) the argument of the logarithm is 2
    np.testing.assert_allclose(ref.custom_softplus(-np.log(9999.0))[0], np.log(2.0), rtol=1e-12)
    # float32, as the device computes it: overflow from x = 79.6 on — value inf, gradient 1
    big = g["x"] > 79.6
    assert big.any() and np.isinf(g["value_f32"][big]).all() and (g["grad_f32"][big] == 1).all()
    assert np.isfinite(g["value_f32"][~big]).all()


def test_abi_9_and_new_symbols():
    from emgraph_amd import _lib as L
    assert L.ABI_VERSION == 9
    header = open(os.path.join(ROOT, "include", "emgraph_hip.h")).read()
    assert re.search(r"#define\s+EMG_ABI_VERSION\s+9\b", header)
    for i, name in enumerate(("LINEAR", "TANH", "SIGMOID", "SOFTPLUS")):
        assert re.search(r"#define\s+EMG_LINK_%s\s+%d\b" % (name, i), header)
        assert getattr(L, "LINK_" + name) == i and L.LINK_IDS[name.lower()] == i
    for sym in ("emg_link_scores", "emg_link_grads"):
        assert sym in L.SIGNATURES and re.search(r"\bint\s+%s\(" % sym, header)
    for cls in (L.BackwardArgs, L.StepArgs):
        names = [f[0] for f in cls._fields_]
        assert names[-3:] == ["link", "sw", "edge_w"], names[-3:]
    assert [f[0] for f in L.PlanConfig._fields_][-4:] == ["link", "reserved2", "edge_w", "link_fac"]
    assert "sw" in [f[0] for f in L.PlanBatch._fields_]
    if os.path.exists(L.LIB_PATH):
        lib = L.load()                                      # (raises unless the library exports every declared symbol at ABI 9)
        assert lib.emg_version() == 9
