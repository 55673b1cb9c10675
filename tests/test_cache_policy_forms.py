"""GPU tests: the cache-policy form of the fused in-place SGD kernel (train_backward_body's CP: non-temporal loads of the
entity rows and stores of the singletons' updates, contribution rows stored plainly) gives the same bits as today's form.
EMG_CACHE_POLICY forces either form, and both legs run in this process: trained tables and epoch losses
are compared byte for byte, and the library's count of cache-policy launches shows which form each leg ran."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _fit(policy, name, k, X, n_ent, n_rel, batches, norm=None, lp=False, loss="nll"):
    from tests.test_api import _models
    old = os.environ.get("EMG_CACHE_POLICY")
    os.environ["EMG_CACHE_POLICY"] = policy
    try:
        rs = np.random.RandomState(5)
        ki = 2 * k if name in ("ComplEx", "HolE") else k
        ent0 = (rs.randn(n_ent, ki) * 0.3).astype(np.float32)
        rel0 = (rs.randn(n_rel, ki) * 0.3).astype(np.float32)
        kw = {}
        if norm is not None:
            kw["embedding_model_params"] = {"norm": norm}
        if lp:
            kw.update(regularizer="LP", regularizer_params={"lambda": 1e-3, "p": 2})
        m = _models()[name](k=k, initializer="constant", initializer_params={"entity": ent0, "relation": rel0}, eta=5, epochs=2,
                            batches_count=batches, seed=11, loss=loss, optimizer="sgd", optimizer_params={"lr": 0.02}, **kw)
        from emgraph_amd import _lib
        lib = _lib.load()
        before = lib.emg_cache_policy_launches()
        m.fit(X)
        ran = lib.emg_cache_policy_launches() - before
        # the form forced is the form that ran: every fused launch here is IP 1 of one wave per group (LP: IP 3, no such form)
        assert (ran > 0) == (policy == "1" and not lp), (policy, lp, ran)
        E, R = m.trained_model_params
        return np.array(E), np.array(R), np.array(m.epoch_losses, dtype=np.float64)
    finally:
        if old is None:
            del os.environ["EMG_CACHE_POLICY"]
        else:
            os.environ["EMG_CACHE_POLICY"] = old


def _same(a, b):
    for x, y, what in zip(a, b, ("entity table", "relation table", "losses")):
        assert x.tobytes() == y.tobytes(), "%s differs" % what


def _uniform(n_ent, n_rel, n, seed=3):
    from tests.test_api import synth_graph
    return synth_graph(n_ent, n_rel, n, seed=seed)


def _zipf(n_ent, n_rel, n, seed=4):
    rs = np.random.RandomState(seed)
    s = np.minimum(rs.zipf(1.3, n) - 1, n_ent - 1)
    o = np.minimum(rs.zipf(1.3, n) - 1, n_ent - 1)
    X = np.stack([s, rs.randint(0, n_rel, n), o], 1)
    X[:n_ent, 0] = np.arange(n_ent)   # every id occurs: ids == labels after the mapping
    X[:n_rel, 1] = np.arange(n_rel)
    return X.astype(np.int64)


@pytest.mark.parametrize("name,k,norm,loss", [("TransE", 100, 1, "pairwise"), ("TransE", 100, 2, "nll"), ("DistMult", 200, None, "nll"),
                                              ("ComplEx", 200, None, "nll"), ("HolE", 100, None, "nll")])
def test_cache_policy_form_gives_the_same_bits_small_table(name, k, norm, loss):
    X = _uniform(900, 7, 2003)
    _same(_fit("1", name, k, X, 900, 7, 6, norm=norm, loss=loss), _fit("0", name, k, X, 900, 7, 6, norm=norm, loss=loss))


@pytest.mark.parametrize("name,k", [("ComplEx", 200), ("TransE", 200)])
def test_cache_policy_form_gives_the_same_bits_wide_batch(name, k):
    """batches past 2048 triples: one wave per group with 50-chunk rows (the C3 kernel's shape), singletons and shared rows"""
    X = _uniform(20000, 50, 24000)
    _same(_fit("1", name, k, X, 20000, 50, 4), _fit("0", name, k, X, 20000, 50, 4))


@pytest.mark.parametrize("name,k", [("ComplEx", 200), ("DistMult", 200)])
def test_cache_policy_form_gives_the_same_bits_zipf_batch(name, k):
    """hub rows: long segments in the apply, few singletons"""
    X = _zipf(20000, 30, 24000)
    _same(_fit("1", name, k, X, 20000, 30, 4), _fit("0", name, k, X, 20000, 30, 4))


def test_cache_policy_switch_leaves_sgd_with_lp_alone():
    """SGD + LP runs its own in-place form (IP 3), which has no cache-policy form: forced on, the form is not launched (_fit checks
    the launch count) and the bits are today's"""
    X = _uniform(900, 7, 2003)
    _same(_fit("1", "ComplEx", 100, X, 900, 7, 6, lp=True), _fit("0", "ComplEx", 100, X, 900, 7, 6, lp=True))
