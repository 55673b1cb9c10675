"""FocusE edge weights and score links on the device, against tests/_focuse_ref.py (a float64 restatement of
EmbeddingModel.py:679-722, 801-816) driven by the device's own Philox draws.

Bars (tests/test_config_widths.py): loss rtol 2e-5; gradients — read back through the SGD update at lr = 0.1 —
rtol 1e-4 with an absolute floor of 2e-7 + 1e-5 x lr x the largest gradient entry; rows no triple touches bit-identical;
fit() tables rtol 2e-3 (tests/test_api.py's fit() bar).  Table scales keep the scores of order one (inside +-75, where the
links are not saturated), and a batch with a pair closer than 2e-5 to a kink of its loss is re-drawn on the host (float32
rounding may take either side of one)."""
import numpy as np
import pytest

from tests import _focuse_ref as ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import emgraph_oracle as orc  # noqa: E402

F32 = np.float32
N_ENT, N_REL, N_TRIPLES, BATCHES = 300, 5, 2047, 4     # batches of 512 and a ragged last one of 511
B = 512
LR = 0.1
SW = 0.25


def _graph(seed=0):
    rs = np.random.RandomState(100 + seed)
    X = np.stack([rs.randint(0, N_ENT, N_TRIPLES), rs.randint(0, N_REL, N_TRIPLES), rs.randint(0, N_ENT, N_TRIPLES)], 1)
    X[:N_ENT, 0] = np.arange(N_ENT)                      # every entity and relation occurs: labels == ids after mapping
    X[:N_REL, 1] = np.arange(N_REL)
    w = rs.uniform(0, 1, N_TRIPLES).astype(F32)          # differs from row to row: a wrong batch offset shows
    return X.astype(np.int64), w


def _tables(model, k, seed):
    """tables whose scores are of order one at any width (module docstring)"""
    rs = np.random.RandomState(seed)
    ki = 2 * k if model in ("ComplEx", "HolE") else k
    sigma = 1.5 / k if model.startswith("TransE") else ((4.0 * k) ** (-1 / 6) if ki != k else float(k) ** (-1 / 6))
    return (rs.randn(N_ENT, ki) * sigma).astype(F32), (rs.randn(N_REL, ki) * sigma).astype(F32), ki


def _mid(model):
    from emgraph_amd import _lib as L
    return L.TRANSE_P if model.startswith("TransE_P") else orc.MODEL_IDS[model]


class _Step:
    """one C-ABI step on fresh copies of the tables: emg_prepare_batch -> scoring -> emg_apply_grouped (SGD)"""

    def __init__(self, model, E0, R0, ki, xb, eta, seed, counter, scale=1.0):
        from emgraph_amd import _lib as L
        from emgraph_amd import device as d
        from emgraph_amd.training import alloc_table
        d.require_gpu()
        self.L, self.d = L, d
        self.model, self.ki, self.eta, self.scale = model, ki, eta, scale
        self.E0, self.R0 = E0, R0
        dev = self.dev = torch.device("cuda")
        self.alloc = lambda a: alloc_table(a.shape[0], ki, dev, init=a)
        nb = len(xb)
        self.nb, self.n_ce = nb, (2 + eta) * nb
        self.pos = torch.from_numpy(np.ascontiguousarray(xb, dtype=np.int32)).to(dev)
        self.we = torch.empty(d.apply_workspace_bytes(self.n_ce, N_ENT, ki), dtype=torch.uint8, device=dev)
        self.wr = torch.empty(d.apply_workspace_bytes(nb, N_REL, ki), dtype=torch.uint8, device=dev)
        self.codes = torch.empty(nb * eta, dtype=torch.int32, device=dev)
        self.de = torch.empty(self.n_ce, dtype=torch.int32, device=dev)
        self.dr = torch.empty(nb, dtype=torch.int32, device=dev)
        self.single = torch.zeros(self.n_ce, dtype=torch.uint8, device=dev)
        self.seed, self.counter = seed, counter

    def _prepare(self, inplace):
        self.d.prepare_batch(self.pos, self.eta, [self.L.SIDE_SO], N_ENT, self.codes, self.de, self.dr, N_ENT, N_REL, self.we,
                             self.wr, seed=self.seed, counter0=self.counter, single_flags=self.single if inplace else None)

    def fused(self, loss, link, w, sw, margin=1.0):
        L, d = self.L, self.d
        Et, Rt = self.alloc(self.E0), self.alloc(self.R0)
        self._prepare(True)
        ce = torch.full((self.n_ce, Et.stride(0)), float("nan"), dtype=torch.float32, device=self.dev)[:, :self.ki]
        cr = torch.full((self.nb, Et.stride(0)), float("nan"), dtype=torch.float32, device=self.dev)[:, :self.ki]
        acc = torch.zeros(1, dtype=torch.float64, device=self.dev)
        hyper = (LR, 0.9, 0.9, 0.999, 1e-7, LR)
        tag_e = torch.zeros(N_ENT, dtype=torch.int32, device=self.dev)
        tag_r = torch.zeros(N_REL, dtype=torch.int32, device=self.dev)
        wt = torch.from_numpy(np.ascontiguousarray(w, dtype=F32)).to(self.dev) if w is not None else None
        sp = torch.empty(self.nb, dtype=torch.float32, device=self.dev)
        sn = torch.empty(self.nb * self.eta, dtype=torch.float32, device=self.dev)
        d.train_backward_ex(_mid(self.model), Et, Rt, self.ki, self.scale, self.pos, self.eta, self.codes, ce, cr,
                            fused_loss=L.LOSS_IDS[loss], margin=margin, loss_accum=acc, single_ent=self.single, opt_id=L.OPT_SGD,
                            step=1, hyper=hyper, tag_ent=tag_e, scores_pos_out=sp, scores_neg_out=sn, link=L.LINK_IDS[link],
                            edge_w=wt, sw=sw)
        d.apply_grouped(L.OPT_SGD, Et, self.ki, None, None, tag_e, 1, ce, self.n_ce, True, hyper, self.we)
        d.apply_grouped(L.OPT_SGD, Rt, self.ki, None, None, tag_r, 1, cr, self.nb, False, hyper, self.wr)
        return Et.cpu().numpy(), Rt.cpu().numpy(), float(acc.item()), sp.cpu().numpy(), sn.cpu().numpy()

    def separate(self, loss, link, w, sw, loss_params=None):
        """emg_train_forward -> emg_link_scores -> emg_loss -> emg_link_grads -> emg_train_backward_ex(fused_loss = -1)"""
        L, d = self.L, self.d
        lp = loss_params or {}
        Et, Rt = self.alloc(self.E0), self.alloc(self.R0)
        self._prepare(False)
        ce = torch.full((self.n_ce, Et.stride(0)), float("nan"), dtype=torch.float32, device=self.dev)[:, :self.ki]
        cr = torch.full((self.nb, Et.stride(0)), float("nan"), dtype=torch.float32, device=self.dev)[:, :self.ki]
        acc = torch.zeros(1, dtype=torch.float64, device=self.dev)
        hyper = (LR, 0.9, 0.9, 0.999, 1e-7, LR)
        tag_e = torch.zeros(N_ENT, dtype=torch.int32, device=self.dev)
        tag_r = torch.zeros(N_REL, dtype=torch.int32, device=self.dev)
        wt = torch.from_numpy(np.ascontiguousarray(w, dtype=F32)).to(self.dev) if w is not None else None
        sp, sn = d.train_forward(_mid(self.model), Et, Rt, self.ki, self.scale, self.pos, self.eta, self.codes)
        fp, fn = d.link_scores(L.LINK_IDS[link], wt, sw, sp, sn, self.nb, self.eta)
        default_margin = 3.0 if loss == "self_adversarial" else 1.0
        gp, gn = d.loss(L.LOSS_IDS[loss], sp, sn, self.nb, self.eta, 1, float(lp.get("margin", default_margin)),
                        float(lp.get("alpha", 0.5)), acc)
        d.link_grads(gp, gn, fp, fn, self.nb, self.eta)
        d.train_backward_ex(_mid(self.model), Et, Rt, self.ki, self.scale, self.pos, self.eta, self.codes, ce, cr, fused_loss=-1,
                            g_pos=gp, g_neg=gn)
        d.apply_grouped(L.OPT_SGD, Et, self.ki, None, None, tag_e, 1, ce, self.n_ce, False, hyper, self.we)
        d.apply_grouped(L.OPT_SGD, Rt, self.ki, None, None, tag_r, 1, cr, self.nb, False, hyper, self.wr)
        return Et.cpu().numpy(), Rt.cpu().numpy(), float(acc.item())


def _compare(E0, R0, E1, R1, loss, terms, xb, x_negs, what):
    np.testing.assert_allclose(loss, terms["loss"], rtol=2e-5, err_msg="loss: " + what)
    for W0, W1, g, tbl in ((E0, E1, terms["dE"], "E"), (R0, R1, terms["dR"], "R")):
        gmax = np.abs(g).max()
        np.testing.assert_allclose(W0.astype(np.float64) - W1, LR * g, rtol=1e-4, atol=2e-7 + 1e-5 * LR * gmax,
                                   err_msg="gradient of %s: %s" % (tbl, what))
    touched = np.zeros(N_ENT, bool)
    for xx in [xb] + list(x_negs):
        touched[xx[:, 0]] = True
        touched[xx[:, 2]] = True
    np.testing.assert_array_equal(E1[~touched], E0[~touched], err_msg="untouched rows: " + what)


def _case(model, k, eta, loss, table_seed, scale=1.0, links=ref.LINKS, weights=(False, True), loss_params=None, sw=SW, n=B):
    """tables, the first batch of the graph, its negatives and the helper's terms for every (link, weights) — the batch re-drawn
    until no pair sits on a kink of the loss"""
    X, w_all = _graph()
    xb, wb = X[:n], w_all[:n]
    for attempt in range(20):
        E0, R0, ki = _tables(model.split(":")[0] if model.startswith("TransE_P") else model, k, table_seed + 1000 * attempt)
        x_negs = ref.negatives(xb, eta, ("s,o",), N_ENT, 11, 1, 1, 1)
        terms = {(lk, ww): ref.step_terms(model, E0, R0, xb, eta, loss, loss_params, x_negs, lk, wb if ww else None, sw, k=k)
                 for lk in links for ww in weights}
        if min(ref.hinge_gap(loss, t, loss_params) for t in terms.values()) > 2e-5:
            assert all(np.abs(t["pos"]).max() < 75 and np.abs(t["negs"][0]).max() < 75 for t in terms.values())
            return E0, R0, ki, xb, wb, x_negs, terms
    raise AssertionError("no batch away from the kinks of the loss")


# ---- 1. the fused step against the helper ----
@pytest.mark.parametrize("loss", ["pairwise", "nll", "absolute_margin"])
@pytest.mark.parametrize("eta", [1, 20])
@pytest.mark.parametrize("k", [3, 50, 200])
@pytest.mark.parametrize("model", ["TransE_L1", "DistMult", "ComplEx"])
def test_fused_step_against_the_helper(model, k, eta, loss):
    E0, R0, ki, xb, wb, x_negs, terms = _case(model, k, eta, loss, table_seed=k + eta)
    st = _Step(model, E0, R0, ki, xb, eta, seed=11, counter=0)
    for (lk, ww), t in terms.items():
        what = "%s k=%d eta=%d %s link=%s weights=%s" % (model, k, eta, loss, lk, ww)
        E1, R1, dev_loss, sp, sn = st.fused(loss, lk, wb if ww else None, SW)
        print(what, "loss", dev_loss, t["loss"])
        _compare(E0, R0, E1, R1, dev_loss, t, xb, x_negs, what)
        # scores_*_out keep receiving the raw scores
        np.testing.assert_allclose(sp, t["pos"], rtol=1e-4, atol=1e-5, err_msg=what)
        np.testing.assert_allclose(sn, t["negs"][0], rtol=1e-4, atol=1e-5, err_msg=what)


def test_fused_step_unit_weights_and_unread_sw_change_no_bit():
    """linear link: the new fields at their zero defaults, a structure weight without weights (not read), and weights that are
    exactly one (the linked form of the kernel) give the same bits as each other"""
    E0, R0, ki, xb, wb, x_negs, terms = _case("ComplEx", 50, 5, "nll", table_seed=1, links=("linear",), weights=(False,))
    st = _Step("ComplEx", E0, R0, ki, xb, 5, seed=11, counter=0)
    a = st.fused("nll", "linear", None, 0.0)
    b = st.fused("nll", "linear", None, 0.7)           # (sw without weights is not read)
    c = st.fused("nll", "linear", np.ones(len(xb), F32), 1.0)   # weights that are exactly one
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    for x, y in zip(a, c):
        np.testing.assert_array_equal(x, y)


def test_softplus_overflows_as_the_reference():
    """a negative scoring 100: 9999 e^100 is inf in float32 — effective score inf, pairwise loss inf, dL/dscore 1 (:90-96)"""
    from emgraph_amd import _lib as L
    from emgraph_amd import device as d
    from emgraph_amd.training import alloc_table
    d.require_gpu()
    dev = torch.device("cuda")
    k = 4
    E0 = np.zeros((3, k), F32)
    R0 = np.zeros((1, k), F32)
    E0[0, 0], E0[1, 0], E0[2, 0], R0[0, 0] = 10.0, 0.1, 10.0, 1.0           # (0, 0, 1) scores 1; object 2 instead: 100
    Et, Rt = alloc_table(3, k, dev, init=E0), alloc_table(1, k, dev, init=R0)
    pos = torch.tensor([[0, 0, 1]], dtype=torch.int32, device=dev)
    we = torch.empty(d.apply_workspace_bytes(3, 3, k), dtype=torch.uint8, device=dev)
    wr = torch.empty(d.apply_workspace_bytes(1, 1, k), dtype=torch.uint8, device=dev)
    codes = torch.empty(1, dtype=torch.int32, device=dev)
    de, dr = torch.empty(3, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    d.prepare_batch(pos, 1, [L.SIDE_O], 3, codes, de, dr, 3, 1, we, wr, inj_repl=torch.tensor([2], dtype=torch.int32, device=dev))
    ce = torch.zeros((3, 4), dtype=torch.float32, device=dev)
    cr = torch.zeros((1, 4), dtype=torch.float32, device=dev)
    acc = torch.zeros(1, dtype=torch.float64, device=dev)
    sn = torch.empty(1, dtype=torch.float32, device=dev)
    sp = torch.empty(1, dtype=torch.float32, device=dev)
    d.train_backward_ex(L.DISTMULT, Et, Rt, k, 1.0, pos, 1, codes, ce, cr, fused_loss=L.LOSS_PAIRWISE, margin=1.0, loss_accum=acc,
                        scores_pos_out=sp, scores_neg_out=sn, link=L.LINK_SOFTPLUS)
    assert float(sn.item()) == 100.0 and abs(float(sp.item()) - 1.0) < 1e-6
    assert np.isinf(acc.item()) and acc.item() > 0
    # dL/dneg = 1 x phi'(100) = 1: the replacement's gradient row is 1 x (p * s) = [10, 0, 0, 0]
    np.testing.assert_array_equal(ce[2].cpu().numpy(), np.array([10, 0, 0, 0], F32))


# ---- 2. the separate path ----
@pytest.mark.parametrize("link", ["tanh", "softplus"])
@pytest.mark.parametrize("model,k,loss", [("DistMult", 50, "self_adversarial"), ("ComplEx", 50, "multiclass_nll"),
                                          ("TransE_P:3", 50, "self_adversarial"), ("TransE_P:3", 33, "multiclass_nll")])
def test_separate_path_against_the_helper(model, k, loss, link):
    eta = 5
    E0, R0, ki, xb, wb, x_negs, terms = _case(model, k, eta, loss, table_seed=7, links=(link,), weights=(True,))
    scale = 3.0 if model.startswith("TransE_P") else 1.0
    st = _Step(model, E0, R0, ki, xb, eta, seed=11, counter=0, scale=scale)
    E1, R1, dev_loss = st.separate(loss, link, wb, SW)
    what = "%s k=%d %s link=%s" % (model, k, loss, link)
    print(what, "loss", dev_loss, terms[(link, True)]["loss"])
    _compare(E0, R0, E1, R1, dev_loss, terms[(link, True)], xb, x_negs, what)


@pytest.mark.parametrize("link", ["tanh", "softplus"])
def test_fused_and_separate_path_agree(link):
    eta = 5
    E0, R0, ki, xb, wb, x_negs, terms = _case("DistMult", 50, eta, "nll", table_seed=9, links=(link,), weights=(True,))
    st = _Step("DistMult", E0, R0, ki, xb, eta, seed=11, counter=0)
    Ef, Rf, lf, _, _ = st.fused("nll", link, wb, SW)
    Es, Rs, ls = st.separate("nll", link, wb, SW)
    t = terms[(link, True)]
    np.testing.assert_allclose(lf, ls, rtol=2e-5)
    for W0, a, b, g in ((E0, Ef, Es, t["dE"]), (R0, Rf, Rs, t["dR"])):
        np.testing.assert_allclose(W0.astype(np.float64) - a, W0.astype(np.float64) - b, rtol=1e-4,
                                   atol=2e-7 + 1e-5 * LR * np.abs(g).max())


# ---- 3 - 6. fit() ----
def _model(name, k, eta, loss, opt, lr, epochs, emp=None, seed=5, **kw):
    from emgraph_amd import models
    E0, R0, _ = _tables(name, k, 40 + k)
    params = {"corrupt_side": "s,o"}
    params.update(emp or {})
    m = getattr(models, name)(k=k, eta=eta, epochs=epochs, batches_count=BATCHES, seed=seed, loss=loss, optimizer=opt,
                              optimizer_params={"lr": lr}, embedding_model_params=params, initializer="constant",
                              initializer_params={"entity": E0, "relation": R0}, **kw)
    return m, E0, R0


@pytest.mark.parametrize("link", ["linear", "sigmoid"])
@pytest.mark.parametrize("name,loss,opt,lr", [("ComplEx", "nll", "adam", 0.01), ("DistMult", "pairwise", "sgd", 0.05)])
def test_fit_end_to_end_against_the_helper(name, loss, opt, lr, link):
    from emgraph_amd.training import focuse_edge_weights
    X, vals = _graph()
    vals = vals.astype(np.float64) * 7 - 2               # raw edge values: normalised per relation by fit()
    k, eta, epochs = 50, 5, 5
    m, E0, R0 = _model(name, k, eta, loss, opt, lr, epochs, emp={"non_linearity": link, "stop_epoch": 4})
    m.fit(X, focusE_numeric_edge_values=vals)
    w = focuse_edge_weights(X[:, 1], vals, seed=5)
    E, R, losses = ref.fit_loop(name, E0, R0, X, w, eta, loss, opt, lr, epochs, BATCHES, ("s,o",), 5, link_name=link, stop_epoch=4,
                                k=k)
    print(name, loss, opt, link, "epoch losses", m.epoch_losses, losses)
    np.testing.assert_allclose(m.trained_model_params[0], E, rtol=2e-3, atol=2e-5)
    np.testing.assert_allclose(m.trained_model_params[1], R, rtol=2e-3, atol=2e-5)
    np.testing.assert_allclose(m.epoch_losses, losses, rtol=2e-3)
    # predict() goes through the link (and not through the weights)
    got = m.predict(X[:64], from_idx=True)
    want = ref.link(link, orc.score_triples(name, m.trained_model_params[0], m.trained_model_params[1], X[:64], k=k))[0]
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("name,loss,opt", [("ComplEx", "nll", "adam"), ("DistMult", "pairwise", "sgd"),
                                           ("DistMult", "self_adversarial", "sgd")])
def test_feature_off_is_really_off(name, loss, opt):
    X, w = _graph()
    runs = []
    for emp, vals in (({}, None), ({"stop_epoch": 0, "structural_wt": 1.0}, w), ({"non_linearity": "linear"}, None)):
        m, _, _ = _model(name, 50, 5, loss, opt, 0.01, 2, emp=emp)
        m.fit(X, focusE_numeric_edge_values=vals)
        runs.append((m.trained_model_params[0].copy(), m.trained_model_params[1].copy(), list(m.epoch_losses)))
    for other in runs[1:]:
        np.testing.assert_array_equal(runs[0][0], other[0])
        np.testing.assert_array_equal(runs[0][1], other[1])
        assert runs[0][2] == other[2]


def test_the_weights_matter():
    X, w = _graph()
    tables = []
    for vals in (w, w[::-1].copy()):
        m, _, _ = _model("DistMult", 50, 5, "nll", "sgd", 0.05, 2, emp={"stop_epoch": 0, "structural_wt": 0.0,
                                                                          "normalize_numeric_values": False})
        m.fit(X, focusE_numeric_edge_values=vals)
        tables.append(m.trained_model_params[0].copy())
    assert np.abs(tables[0] - tables[1]).max() > 1e-4
    # The positive's gradient scales with 1 - w_i.  absolute_margin with a margin no negative reaches: the negatives get no
    # gradient, dL/d(effective positive) = -eta, so dL/dpos_i = -eta (1 - w_i) at structure weight 0; every positive has a
    # relation of its own, whose row then moves by exactly that times s * o.
    from emgraph_amd import _lib as L
    from emgraph_amd import device as d
    from emgraph_amd.training import alloc_table
    dev = torch.device("cuda")
    nb, k, eta = 64, 8, 3
    rs = np.random.RandomState(3)
    E0, R0 = (rs.randn(N_ENT, k) * 0.5).astype(F32), (rs.randn(nb, k) * 0.5).astype(F32)
    xb = np.stack([rs.randint(0, N_ENT, nb), np.arange(nb), rs.randint(0, N_ENT, nb)], 1).astype(np.int32)
    wb = rs.uniform(0, 1, nb).astype(F32)
    Et, Rt = alloc_table(N_ENT, k, dev, init=E0), alloc_table(nb, k, dev, init=R0)
    pos = torch.from_numpy(xb).to(dev)
    n_ce = (2 + eta) * nb
    we = torch.empty(d.apply_workspace_bytes(n_ce, N_ENT, k), dtype=torch.uint8, device=dev)
    wr = torch.empty(d.apply_workspace_bytes(nb, nb, k), dtype=torch.uint8, device=dev)
    codes = torch.empty(nb * eta, dtype=torch.int32, device=dev)
    de, dr = torch.empty(n_ce, dtype=torch.int32, device=dev), torch.empty(nb, dtype=torch.int32, device=dev)
    d.prepare_batch(pos, eta, [L.SIDE_SO], N_ENT, codes, de, dr, N_ENT, nb, we, wr, seed=1, counter0=0)
    ce = torch.zeros((n_ce, 8), dtype=torch.float32, device=dev)
    cr = torch.zeros((nb, 8), dtype=torch.float32, device=dev)
    acc = torch.zeros(1, dtype=torch.float64, device=dev)
    d.train_backward_ex(L.DISTMULT, Et, Rt, k, 1.0, pos, eta, codes, ce, cr, fused_loss=L.LOSS_ABSOLUTE_MARGIN, margin=-1000.0,
                        loss_accum=acc, edge_w=torch.from_numpy(wb).to(dev), sw=0.0)
    x_negs = ref.negatives(xb, eta, ("s,o",), N_ENT, 1, 1, 1, 1)
    t = ref.step_terms("DistMult", E0, R0, xb, eta, "absolute_margin", {"margin": -1000.0}, x_negs, "linear", wb, 0.0, k=k)
    np.testing.assert_allclose(t["g_pos"], -eta * (1 - wb.astype(np.float64)), rtol=1e-12)
    want = t["g_pos"][:, None] * (E0[xb[:, 0]].astype(np.float64) * E0[xb[:, 2]])
    np.testing.assert_allclose(cr.cpu().numpy(), want, rtol=1e-4, atol=1e-6)


def test_refusals():
    from emgraph_amd.evaluation import evaluate_performance
    X, w = _graph()
    m, _, _ = _model("DistMult", 8, 2, "nll", "sgd", 0.01, 1, emp={"non_linearity": "tanh"})
    m.fit(X)
    with pytest.raises(NotImplementedError):
        evaluate_performance(X[:8], m, filter_triples=X)
    with pytest.raises(NotImplementedError):
        m.fit(X, early_stopping=True, early_stopping_params={"x_valid": X[:8]})
    for sharding in ("k", "batch"):
        m2, _, _ = _model("DistMult", 8, 2, "nll", "sgd", 0.01, 1, emp={"sharding": sharding})
        with pytest.raises(NotImplementedError):
            m2.fit(X, focusE_numeric_edge_values=w)
        m3, _, _ = _model("DistMult", 8, 2, "nll", "sgd", 0.01, 1, emp={"sharding": sharding, "non_linearity": "sigmoid"})
        with pytest.raises(NotImplementedError):
            m3.fit(X)
    m4, _, _ = _model("DistMult", 8, 2, "nll", "sgd", 0.01, 1, emp={"non_linearity": "relu"})
    with pytest.raises(ValueError, match="Invalid non-linearity"):
        m4.fit(X)
    # a FocusE model under the default linear link is ranked by the existing evaluation
    m5, _, _ = _model("DistMult", 8, 2, "nll", "sgd", 0.01, 1)
    m5.fit(X, focusE_numeric_edge_values=w)
    ranks = evaluate_performance(X[:8], m5, filter_triples=X)
    assert np.asarray(ranks).size >= 8
