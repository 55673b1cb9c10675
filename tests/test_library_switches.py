"""GPU tests: the library's A/B switches that claim "same bits" give the same bits.  Every leg sets its switches and fits in this
process (a small fit — untouched rows, singletons and shared rows in every step — whose trained tables, optimizer state and epoch
losses are compared byte for byte).
  EMG_DENSE_FUSED  Keras Adam's dense-equivalent pass over the untouched rows inside the descriptor-driven apply launch / as a
                   launch of its own (emg_apply.hip: ApplyParams.dense_here)
  EMG_APPLY_FIX    the apply's optimizer rule fixed at compile time / the run-time switch (apply_segments_kernel<..., FIX>)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _run(monkeypatch, env_over, name, k, loss, opt, lp=None):
    from tests.test_api import _models, synth_graph
    reg = {} if lp is None else dict(regularizer="LP", regularizer_params={"lambda": 1e-3, "p": lp})
    n_ent, n_rel, n = 900, 7, 2003   # 6 batches of 334 / 333 triples, eta 5: ~4000 slots over 900 rows — touched and untouched rows in every step
    X = synth_graph(n_ent, n_rel, n, seed=3)
    rs = np.random.RandomState(5)
    ki = 2 * k if name in ("ComplEx", "HolE") else k
    ent0 = (rs.randn(n_ent, ki) * 0.3).astype(np.float32)
    rel0 = (rs.randn(n_rel, ki) * 0.3).astype(np.float32)
    with monkeypatch.context() as mp:   # (the leg's switches only: the Trainer's plan and every launch are made inside fit)
        mp.setenv("EMG_GRAPH", "1")
        for key, val in env_over.items():
            mp.setenv(key, val)
        m = _models()[name](k=k, initializer="constant", initializer_params={"entity": ent0, "relation": rel0}, eta=5, epochs=2,
                            batches_count=6, seed=11, loss=loss, optimizer=opt, optimizer_params={"lr": 0.02}, **reg)
        m.fit(X)
        E, R = m.trained_model_params
        out = dict(E=np.array(E), R=np.array(R), losses=np.array(m.epoch_losses, dtype=np.float64))
        tr = m._trainer
        for nm in ("state_ent", "state_rel"):
            st = getattr(tr, nm, None)
            if st:
                for i, t in enumerate(st):
                    if t is not None:
                        out["%s%d" % (nm, i)] = t.detach().cpu().numpy()
    return out


def _same(a, b):
    assert sorted(a) == sorted(b)
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), "%s differs" % key


@pytest.mark.parametrize("name,k,loss", [("TransE", 100, "pairwise"),      # rows of 25 chunks: two segments per wave
                                         ("DistMult", 200, "nll"),         # 50 chunks: a wave per segment, factored contributions
                                         ("ComplEx", 100, "nll")])
def test_adam_dense_pass_inside_the_apply_launch_gives_the_same_bits(monkeypatch, name, k, loss):
    a = _run(monkeypatch, {"EMG_DENSE_FUSED": "1"}, name, k, loss, "adam")
    b = _run(monkeypatch, {"EMG_DENSE_FUSED": "0"}, name, k, loss, "adam")
    assert "state_ent1" in a   # (Adam's second moments were dumped: the comparison covers m and v)
    _same(a, b)


@pytest.mark.parametrize("name,k,loss,opt", [("TransE", 100, "pairwise", "adam"), ("DistMult", 200, "nll", "adam"),
                                             ("ComplEx", 100, "nll", "adagrad"), ("TransE", 100, "nll", "adagrad")])
def test_compile_time_optimizer_forms_of_the_apply_give_the_same_bits(monkeypatch, name, k, loss, opt):
    a = _run(monkeypatch, {"EMG_APPLY_FIX": "1"}, name, k, loss, opt)
    b = _run(monkeypatch, {"EMG_APPLY_FIX": "0"}, name, k, loss, opt)
    _same(a, b)
    c = _run(monkeypatch, {"EMG_APPLY_FIX": "1", "EMG_GRAPH": "0"}, name, k, loss, opt)   # (and as single steps)
    _same(a, c)


@pytest.mark.parametrize("name,k,loss,p", [("ComplEx", 100, "nll", 2), ("DistMult", 200, "pairwise", 2), ("TransE", 100, "nll", 3)])
def test_sgd_with_the_lp_regulariser_folds_the_same_bits_in_every_form(monkeypatch, name, k, loss, p):
    """plain SGD + LP: the apply's compile-time form for p = 2 (apply_segments_kernel<..., kFixSgdLp2>) against the run-time switch,
    and the two-multiplication fold lp_fold_p2 that every p = 2 path takes since round 5 (lambda 2 |w| sgn w = fl(2 lambda w)) — the
    tables byte for byte; the regulariser's value is a sum of float partials added as double atomics from several kernels: equal to 1e-9.  p = 3 keeps the
    generic fold in both legs (the switch must not touch it)."""
    a = _run(monkeypatch, {"EMG_APPLY_FIX": "1"}, name, k, loss, "sgd", lp=p)
    b = _run(monkeypatch, {"EMG_APPLY_FIX": "0"}, name, k, loss, "sgd", lp=p)
    c = _run(monkeypatch, {"EMG_APPLY_FIX": "1", "EMG_INPLACE": "0", "EMG_GRAPH": "0"}, name, k, loss, "sgd", lp=p)   # every row through the apply
    for other in (b, c):
        for key in ("E", "R"):
            assert a[key].tobytes() == other[key].tobytes(), "%s differs" % key
        np.testing.assert_allclose(a["losses"], other["losses"], rtol=1e-9)   # (float partials per wave, added as doubles: the partition of the rows over the waves differs between the forms)
