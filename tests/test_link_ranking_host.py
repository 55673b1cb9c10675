"""Ranking through the score link, host side: the opt-in key, the refusals that stay, the ABI table, and the float64 interval
restatement of the reference's semantics (tests/_link_rank_ref.py) on the golden rank tables."""
import os
import re

import numpy as np
import pytest

from tests import _link_rank_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = {"emg_eval_build_queries_link": 17, "emg_eval_count_link": 16, "emg_eval_filter_count_link": 18,
               "emg_eval_rescore_pairs_link": 19, "emg_eval_link_thresholds": 9, "emg_eval_prefilter_f16_thr4": 15,
               "emg_eval_link_order_violations": 6, "emg_eval_link_order_w": 1}


def _model(emp):
    from emgraph_amd import models
    return models.DistMult(k=4, eta=1, epochs=1, batches_count=1, embedding_model_params=emp)


def test_key_parsing():
    assert _model({})._rank_through_link() is False
    assert _model({"rank_through_link": False})._rank_through_link() is False
    assert _model({"rank_through_link": True})._rank_through_link() is True
    assert _model({"rank_through_link": np.bool_(True)})._rank_through_link() is True
    for bad in (1, 0, "True", "yes", None, 1.0):
        with pytest.raises(ValueError, match="rank_through_link"):
            _model({"rank_through_link": bad, "non_linearity": "tanh"})._refuse_ranking_under_link("ranking")
        with pytest.raises(ValueError, match="rank_through_link"):   # a bad value is an error under the linear link too
            _model({"rank_through_link": bad})._refuse_ranking_under_link("ranking")


@pytest.mark.parametrize("link", ["tanh", "sigmoid", "softplus"])
def test_refusals_without_the_key_and_what_the_key_opens(link):
    from emgraph_amd import _lib as L
    for emp in ({"non_linearity": link}, {"non_linearity": link, "rank_through_link": False}):
        m = _model(emp)
        for what in ("ranking (get_ranks, evaluate_performance)", "early stopping", "discover_facts"):
            with pytest.raises(NotImplementedError, match="non_linearity") as ei:
                m._refuse_ranking_under_link(what)
            assert "rank_through_link" in str(ei.value) and what in str(ei.value)
    m = _model({"non_linearity": link, "rank_through_link": True})
    m._refuse_ranking_under_link("ranking")                        # passes
    assert m._rank_link_id() == L.LINK_IDS[link]
    with pytest.raises(NotImplementedError, match="non_linearity"):   # the grid kernel does not carry the link: refused anyway
        m._refuse_ranking_under_link("discover_facts", always=True)
    # the key has no effect under the linear link
    for emp in ({}, {"rank_through_link": True}, {"non_linearity": "linear", "rank_through_link": True}):
        m = _model(emp)
        m._refuse_ranking_under_link("ranking")
        m._refuse_ranking_under_link("discover_facts", always=True)
        assert m._rank_link_id() == L.LINK_LINEAR


def test_discover_facts_stays_refused_with_the_key():
    from emgraph_amd import discovery
    X = np.array([["a", "r", "b"], ["b", "r", "c"]])
    for emp in ({"non_linearity": "tanh", "rank_through_link": True}, {"non_linearity": "tanh"}):
        m = _model(emp)
        m.ent_to_idx, m.rel_to_idx, m.is_fitted = {"a": 0, "b": 1, "c": 2}, {"r": 0}, True
        with pytest.raises(NotImplementedError, match="non_linearity"):
            discovery.discover_facts(X, m, top_n=2, strategy="random_uniform", max_candidates=4, seed=0)


def test_abi_table_has_the_new_symbols():
    from emgraph_amd import _lib as L
    assert L.ABI_VERSION == 9
    hdr = open(os.path.join(ROOT, "include", "emgraph_hip.h")).read()
    assert re.search(r"#define EMG_ABI_VERSION 9\b", hdr)
    for sym, n_args in NEW_SYMBOLS.items():
        m = re.search(r"\bint(?:32_t)?\s+%s\(([^;]*)\);" % sym, hdr)
        assert m, sym
        assert len(m.group(1).split(",")) == n_args == len(L.SIGNATURES[sym][1]), sym
    if os.path.exists(L.LIB_PATH):
        lib = L.load()
        for sym in NEW_SYMBOLS:
            assert hasattr(lib, sym), sym
        assert [lib.emg_eval_link_order_w(i) for i in (-1, 0, 4)] == [-1, 1, -1]
        for link in (L.LINK_TANH, L.LINK_SIGMOID, L.LINK_SOFTPLUS):
            assert lib.emg_eval_link_order_w(link) in (0, 1, 2, 4, 8, 16, 32)


def test_host_resolution_of_the_precision_under_a_link():
    """TransE takes precision 0 under a link; the contraction models keep the exact-fast mode where the link has an order slack"""
    from emgraph_amd import _lib as L
    from emgraph_amd.evaluation import ranking as RK
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("library not built")
    for model in (L.TRANSE_L1, L.TRANSE_L2, L.TRANSE_P):
        assert RK.resolve_auto_precision(model, 200, 4096, 1 << 20, None, L.LINK_TANH) == 0
        assert not RK.link_prefilter_applies(model, L.LINK_TANH)
        assert RK.link_prefilter_applies(model, L.LINK_LINEAR)
    assert RK.resolve_auto_precision(L.TRANSE_L1, 200, 4096, 1 << 20) == 2          # unchanged without a link
    for link in (L.LINK_TANH, L.LINK_SIGMOID, L.LINK_SOFTPLUS):
        want = 2 if RK.D.link_order_w(link) > 0 else 0
        assert RK.resolve_auto_precision(L.COMPLEX, 400, 4096, 1 << 20, None, link) == want
        assert RK.resolve_auto_precision(L.COMPLEX, 400, 4096, 1 << 20, [1, 2, 3], link) == 0
    with pytest.raises(ValueError, match="link"):
        RK.rank_triples_device(L.DISTMULT, None, None, 4, 1.0, np.zeros((1, 3), np.int32), link=7)


def _golden_lists(g):
    return dict(obj_ptr=g["flt_obj_ptr"], obj_idx=g["flt_obj_idx"], sub_ptr=g["flt_sub_ptr"], sub_idx=g["flt_sub_idx"])


@pytest.mark.parametrize("name", ["TransE", "DistMult", "ComplEx", "HolE"])
def test_the_helper_restates_the_reference_on_the_linear_link(golden, name, monkeypatch):
    """the helper's raw scores and rank assembly against the reference's own execution (tests/golden/ranks.npz, 'worst'): with the
    identity in place of the link every interval must hold the golden rank, raw and filtered"""
    g = golden("ranks")
    monkeypatch.setattr(ref, "phi64", lambda link, x: x)
    E, R, T = g["rk_%s_E" % name], g["rk_%s_R" % name], g["flt_test"]
    assert len(T) == 20
    for exp, lists in ((g["rk_%s_worst_raw" % name], {}), (g["rk_%s_worst_s,o" % name], _golden_lists(g))):
        lo, hi = ref.rank_intervals(name, "tanh", E, R, T, **lists)
        assert ((lo <= exp) & (exp <= hi)).all()
        assert (lo == hi).sum() >= 30


@pytest.mark.parametrize("link", ref.LINKS)
@pytest.mark.parametrize("name", ["TransE", "DistMult", "ComplEx", "HolE"])
def test_the_interval_pin_is_not_vacuous(golden, name, link):
    """at least 30 of the 40 (triple, side) rows have rank_lo == rank_hi (unfiltered 'worst' ranks on the golden tables)"""
    g = golden("ranks")
    lo, hi = ref.rank_intervals(name, link, g["rk_%s_E" % name], g["rk_%s_R" % name], g["flt_test"])
    assert lo.shape == (20, 2) and (lo <= hi).all() and (lo >= 1).all()
    tight = int((lo == hi).sum())
    print(name, link, "tight rows:", tight, "of 40; widest:", int((hi - lo).max()))
    assert tight >= 30
