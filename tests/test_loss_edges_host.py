"""CPU tests of tests/_loss_edge_ref.py: the grid keeps its kinks, the literal float32 restatement is the reference's (golden
fixture, oracle.loss_apply), the class table, and the error budget the GPU tests hold the device to — derived here, printed per
loss and per link, and bounded (a budget of 16 ulp or more means the derivation is wrong, not the kernel)."""
import numpy as np
import pytest

from oracle import emgraph_oracle as orc
from tests import _loss_edge_ref as ref

F32 = np.float32
G = ref.GRID


def _shapes():
    """(label, pos, neg, eta, n_sides): the finite and the non-finite shapes of tests/test_loss_edges.py"""
    yield ("pairs",) + ref.all_pairs() + (1, 1)
    yield ("eta3x2",) + ref.drawn(3, 2) + (3, 2)
    yield ("eta70",) + ref.drawn(70, 1) + (70, 1)
    yield ("nonfinite pairs",) + ref.nonfinite_pairs() + (1, 1)
    yield ("nonfinite eta3",) + ref.nonfinite_drawn(3) + (3, 1)


def test_the_grid_keeps_its_kinks():
    assert G.dtype == F32 and len(G) == 43 and np.isfinite(G).all()
    np.testing.assert_array_equal(G, -G[::-1])
    assert (np.diff(G) > 0).all()
    for v in (2.0 ** -140, 75.0, np.nextafter(F32(75), F32(0)), np.nextafter(F32(75), F32(np.inf)), 79, 80, 88, 89, 104, 3e38):
        assert F32(v) in G and -F32(v) in G
    assert set(ref.MUST_KEEP.tolist()) <= set(G.tolist())
    pos, neg = ref.all_pairs()
    with np.errstate(over="ignore"):
        v = (F32(1) - pos) + neg                       # pairwise.py:69 at margin 1, float32
    # 23 pairs exactly on the kink, 983 active, 843 inactive — 2 of them (+-3e38 against -+3e38) with a v past float32
    assert (int((v == 0).sum()), int((v > 0).sum()), int((v < 0).sum()), int((~np.isfinite(v)).sum())) == (23, 983, 843, 2)
    v = F32(1) + G                                     # absolute_margin.py:69
    assert (int((v == 0).sum()), int((v > 0).sum()), int((v < 0).sum())) == (1, 25, 17)
    assert len(ref.NONFINITE) == 4 and np.signbit(ref.NONFINITE[0]) and ref.NONFINITE[0] == 0


def test_the_literal_restatement_is_the_references(golden):
    g = golden("losses")
    for ci, (eta, B) in enumerate(g["cases"]):
        eta = int(eta)
        pos, neg = g["c%d_pos" % ci], g["c%d_neg" % ci]
        for name in ref.KINDS:
            if name in orc.REQUIRE_SAME_SIZE:
                got = ref.terms32(name, pos, neg, eta).astype(np.float64).sum()
                np.testing.assert_allclose(got, g["c%d_%s" % (ci, name)], rtol=1e-5, err_msg="%s c%d" % (name, ci))
        got = ref.terms32("self_adversarial", pos, neg, eta, {"margin": 1.0, "alpha": 2.0}).astype(np.float64).sum()
        np.testing.assert_allclose(got, g["c%d_self_adversarial_m1_a2" % ci], rtol=1e-5)
    rs = np.random.RandomState(0)
    for eta in (1, 4):
        pos, neg = (rs.randn(50) * 20).astype(F32), (rs.randn(50 * eta) * 20).astype(F32)
        for name, params in ref.LOSS_CONFIGS:
            pos_in = np.tile(pos, eta) if orc.REQUIRE_SAME_SIZE[name] else pos
            with np.errstate(over="ignore"):
                want = orc.loss_apply(name, pos_in, neg, eta, params)
            np.testing.assert_allclose(ref.terms32(name, pos, neg, eta, params).astype(np.float64).sum(), want, rtol=1e-5, err_msg=name)
            gp, gn = ref.grads32(name, pos, neg, eta, params)
            wp, wn = orc.loss_grads(name, pos, neg, eta, params)
            np.testing.assert_allclose(gp, wp, rtol=1e-5, atol=1e-6, err_msg=name)
            np.testing.assert_allclose(gn, wn, rtol=1e-5, atol=1e-6, err_msg=name)


def test_the_oracle_hands_a_nan_score_on_under_every_loss():
    for name, params in ref.LOSS_CONFIGS:
        for pos, neg in (([np.nan], [0.5]), ([0.5], [np.nan])):
            pos, neg = np.array(pos, F32), np.array(neg, F32)
            assert np.isnan(orc.loss_apply(name, pos, neg, 1, params)), name                # losses/utils.py:49: clip_by_value
            assert np.isnan(ref.terms32(name, pos, neg, 1, params)[0]), name


def test_the_class_table():
    inf, nan = F32(np.inf), F32(np.nan)
    # pos -75 with three negatives at +75 under multiclass: e^-75 / (e^-75 + 3 e^75) underflows to 0, the loss is -log 0
    t = ref.terms32("multiclass_nll", [-75], [75, 75, 75], 3)
    assert t[0] == inf
    gp, gn = ref.grads32("multiclass_nll", [-75], [75, 75, 75], 3)
    assert gp[0] == -1 and np.allclose(gn, 1 / 3)
    # the first float outside the clip: no gradient; the bound itself: inside
    gp, gn = ref.grads32("nll", [75, np.nextafter(F32(75), inf)], [-75, np.nextafter(F32(-75), -inf)], 1)
    assert gp[0] < 0 and gp[1] == 0 and gn[0] > 0 and gn[1] == 0
    # tf.maximum's gradient at the kink goes to the hinge (MaximumGrad: x >= y)
    assert ref.grads32("pairwise", [1.5], [0.5], 1, {"margin": 1.0})[1][0] == 1
    assert ref.grads32("absolute_margin", [0], [-1], 1, {"margin": 1.0})[1][0] == 1
    # pairwise past float32: 1 + 3e38 + 3e38
    assert ref.terms32("pairwise", [-3e38], [3e38], 1)[0] == inf and ref.terms32("pairwise", [3e38], [-3e38], 1)[0] == 0
    # a one-hot softmax, and a group of all -3e38 (softmax uniform, every log-sigmoid term -0)
    gp, gn = ref.grads32("self_adversarial", [0], [-1e4, 1e4, -1e4], 3)
    np.testing.assert_array_equal(gn, [0, 1, 0])
    gp, gn = ref.grads32("self_adversarial", [0], [-3e38] * 3, 3)
    np.testing.assert_array_equal(gn, [0, 0, 0])
    # links: softplus at 80 (9999 e^80 is inf in float32): value inf, derivative 1; saturated tanh and sigmoid: derivative 0
    s, d = ref.link32("softplus", [79, 80])
    assert np.isfinite(s[0]) and s[1] == inf and d[1] == 1
    assert ref.link32("tanh", [76])[1][0] == 0 and ref.link32("sigmoid", [104, -104])[1].tolist() == [0, 0]
    s, d = ref.link32("softplus", [80], weight=np.zeros(1, F32))
    assert np.isnan(s[0]) and d[0] == 0
    for name in ref.LINKS:
        s, d = ref.link32(name, [nan])
        assert np.isnan(s[0])
    assert ref.class_of_sum([1.0, inf]) == 1 and ref.class_of_sum([inf, -inf]) == 3 and ref.class_of_sum([nan, 1]) == 3


def test_the_float64_restatement_is_the_oracles():
    """grads64 keeps oracle.loss_grads' formulas in float64 to the end (the oracle rounds its result to float32); on scores where
    the self-adversarial exponents are exact in float32 (multiples of 1/4, alpha 0.5 and 1) the two agree to that rounding"""
    rs = np.random.RandomState(1)
    for eta in (1, 3):
        pos, neg = (rs.randint(-40, 41, 60) / 4).astype(F32), (rs.randint(-40, 41, 60 * eta) / 4).astype(F32)
        for name, params in ref.LOSS_CONFIGS:
            gp, gn, _, _ = ref.grads64(name, pos, neg, eta, params)
            wp, wn = orc.loss_grads(name, pos, neg, eta, params)
            np.testing.assert_allclose(gp, wp, rtol=1.2e-7, atol=1e-45, err_msg=name)
            np.testing.assert_allclose(gn, wn, rtol=1.2e-7, atol=1e-45, err_msg=name)


def test_the_budget_is_finite_and_small():
    """printed: the largest budget per loss and side, in ulps of the cancellation-free magnitude"""
    worst = {}
    kept = total = 0
    for label, pos, neg, eta, n_sides in _shapes():
        for name, params in ref.LOSS_CONFIGS:
            for side, e in zip(("g_pos", "g_neg"), ref.loss_expect(name, pos, neg, eta, params, n_sides)):
                fin = e.finite()
                assert np.isfinite(e.tol[fin]).all() and np.isfinite(e.want[fin]).all(), (label, name, side)
                normal = fin & (np.abs(e.want) >= np.finfo(F32).tiny)
                if side == "g_neg":       # (a denormal softmax weight is as short of bits as a denormal gradient)
                    normal &= ref.softmax_weight_normal(name, pos, neg, eta, params, n_sides)
                assert (e.ulps[normal] < 16).all(), (label, name, side, e.ulps[normal].max())
                if name in ("pairwise", "absolute_margin"):
                    assert (e.tol[fin] == 0).all()            # small integers: ==
                if normal.any():
                    worst[(name, side)] = max(worst.get((name, side), 0.0), float(e.ulps[normal].max()))
                kept += int(fin.sum())
                total += int(np.isfinite(e.lit).sum())
    for k in sorted(worst):
        print("budget %-17s %s: %.2f ulp" % (k[0], k[1], worst[k]))
    # no grid point is skipped silently: all that is not asserted is the gradient at a NaN score
    print("asserted by value: %d of %d elements whose literal float32 class is finite" % (kept, total))
    assert kept >= 0.95 * total
    # orientation: the unperturbed NLL dL/dneg chain against float64, on all pairs
    pos, neg = ref.all_pairs()
    lit = ref.grads32("nll", pos, neg, 1)[1].astype(np.float64)
    want = ref.grads64("nll", pos, neg, 1)[1]
    nz = want != 0
    print("unperturbed NLL dL/dneg: %.2f ulp" % (np.abs(lit - want)[nz] / ref.ulp_of(want)[nz]).max())


def test_the_link_budget_is_finite_and_small():
    """printed: the largest budget per link, without and with FocusE weights (the edge weights and structure weights of the GPU test)"""
    x = np.repeat(ref.FULL, 4).astype(F32)
    w = np.tile(np.array([0, 2.0 ** -20, 0.5, 1], F32), len(ref.FULL))
    cases = [("no weights", None)] + [("weights", ref.weight32(sw, w, positive)) for sw in (0.0, 0.25, 1.0) for positive in (True, False)]
    for name in ref.LINKS:
        worst = {}
        for label, weight in cases:
            es, ed = ref.link_expect(name, x, weight)
            for what, e in (("value", es), ("derivative", ed)):
                fin = e.finite()
                assert np.isfinite(e.tol[fin]).all()
                normal = fin & (np.abs(e.want) >= np.finfo(F32).tiny)
                assert (e.ulps[normal] < 16).all(), (name, what, e.ulps[normal].max())
                worst[(label, what)] = max(worst.get((label, what), 0.0), float(e.ulps[normal].max()))
            if name == "linear" and weight is None:
                assert (es.tol[es.finite()] == 0).all() and (ed.tol[ed.finite()] == 0).all()
        print("budget link %-8s value / derivative: %.2f / %.2f ulp; with weights %.2f / %.2f ulp" % (
            name, worst[("no weights", "value")], worst[("no weights", "derivative")], worst[("weights", "value")],
            worst[("weights", "derivative")]))


def test_the_three_launches_cover_every_group():
    for label, pos, neg, eta, n_sides in _shapes():
        for name, params in ref.LOSS_CONFIGS:
            a, b, c = ref.split_groups(name, pos, neg, eta, params, n_sides)
            assert ((a.astype(int) + b + c) == 1).all()
            if label == "pairs":
                assert a.sum() == 17 * 17 and b.sum() > 1000
                if name == "pairwise":        # 1 + 3e38 + 3e38 = inf; its mirror image is -inf, a term of 0
                    assert c.sum() == 1
            for m in (a, b):                        # the float64 sums the first two launches are compared with are finite
                if m.any():
                    p, n = ref.take_groups(pos, neg, eta, n_sides, m)
                    assert np.isfinite(ref.loss_sum64(name, p, n, eta, params, n_sides)).all(), (label, name)
