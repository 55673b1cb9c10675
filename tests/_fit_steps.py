"""fit() one optimizer step at a time, each step checked against the oracle from the device's OWN pre-step state.

``record_steps(monkeypatch)`` replaces ``Trainer.run_batches`` with the non-graph branch's loop (one ``step()`` per batch, the next
three batches prefetched, training.py ``run_batches``) and snapshots after every step: the tables, the unpadded optimizer state, the
step count and the cumulative loss (``read_loss(reset=False)``; fit() resets it after each epoch, so a step's loss is the difference
to the snapshot before it within its epoch).

``_random_fit_config(seed)`` is the soak's configuration of a seed (tests/test_api.py's two fit() soaks, tools/dbg_fuzz_seed.py).

``check_step_by_step(cfg, monkeypatch)`` fits such a configuration that way, fits it again on the
default path (graph replays included) and asks for the same bits, then checks every step: with the float64 gradient of the
pre-step tables and its allowances (``orc.train_grads_bounds``: rounding A, jumps J) every table and state element must lie in
``orc.opt_apply_interval`` over [g - A - J, g + A + J] (+- 2 ulp of the result, of the value before and of the change: the last roundings of the update), Adam's table within a few
ulps of the update the step's own moments give, rows the oracle leaves alone bit-identical, the step's loss within its allowance
and at most 1 % of the touched elements excused by a jump (inside the interval of A + J, outside that of A alone).  Nothing carries over from step to step: each update is held to its own
rounding scale."""
import numpy as np

from oracle import emgraph_oracle as orc

F32 = np.float32


def _random_fit_config(seed):
    """the random fit() configuration of soak seed ``seed`` (both soaks below, tools/dbg_fuzz_seed.py): model / width / eta / loss /
    optimizer / corruption-side list / graph shape (uniform or hub-heavy) / LP regulariser, the mapped training set, the initial
    tables and the model's keyword arguments"""
    rs = np.random.RandomState(7000 + seed)
    name = str(rs.choice(["TransE", "TransE", "DistMult", "ComplEx", "HolE"]))
    norm = int(rs.choice([1, 2]))
    k = int(rs.choice([3, 5, 8, 13, 16, 24, 33, 50, 64, 100, 130, 200, 260]))
    eta = int(rs.choice([1, 2, 3, 5, 10, 20]))
    loss = str(rs.choice(["pairwise", "nll", "absolute_margin", "self_adversarial", "multiclass_nll"]))
    opt = str(rs.choice(["sgd", "momentum", "adagrad", "adam"]))
    sides = [("s,o",), ("s", "o"), ("o",), ("s",), ("s+o",)][rs.randint(0, 5)]
    n_ent, n_rel = int(rs.randint(20, 1500)), int(rs.randint(1, 9))
    n, bc, epochs, lr = int(rs.randint(60, 900)), int(rs.randint(1, 5)), int(rs.randint(1, 3)), float(rs.choice([0.01, 0.05]))
    if rs.randint(0, 2):   # hub-heavy subjects / objects: long segments in the apply
        w = 1.0 / np.arange(1, n_ent + 1)
        w /= w.sum()
        X = np.stack([rs.choice(n_ent, n, p=w), rs.randint(0, n_rel, n), rs.choice(n_ent, n, p=w)], 1)
    else:
        X = np.stack([rs.randint(0, n_ent, n), rs.randint(0, n_rel, n), rs.randint(0, n_ent, n)], 1)
    ids = np.unique(np.concatenate([X[:, 0], X[:, 2]]))                       # labels == ids after the np.unique mapping
    remap = np.full(n_ent, -1, np.int64)
    remap[ids] = np.arange(len(ids))
    X = np.stack([remap[X[:, 0]], X[:, 1], remap[X[:, 2]]], 1).astype(np.int64)
    rels = np.unique(X[:, 1])
    X[:, 1] = np.searchsorted(rels, X[:, 1])
    n_ent, n_rel = len(ids), len(rels)
    ki = 2 * k if name in ("ComplEx", "HolE") else k
    ent0 = (rs.randn(n_ent, ki) * 0.3).astype(F32)
    rel0 = (rs.randn(n_rel, ki) * 0.3).astype(F32)
    emp = {"corrupt_side": list(sides) if len(sides) > 1 else sides[0]}
    if name == "TransE":
        emp["norm"] = norm
    reg, reg_kw = None, {}
    if rs.randint(0, 3) == 0:                                # LP regulariser over the FULL tables (regularizers/lp.py:81-113)
        reg = {"lam": float(rs.choice([0.001, 0.01])), "p": int(rs.choice([1, 2, 3]))}
        reg_kw = dict(regularizer="LP", regularizer_params={"lambda": reg["lam"], "p": reg["p"]})
    kw = dict(k=k, eta=eta, epochs=epochs, batches_count=bc, seed=seed, loss=loss, optimizer=opt, optimizer_params={"lr": lr},
              embedding_model_params=emp, initializer="constant", initializer_params={"entity": ent0, "relation": rel0}, **reg_kw)
    return dict(seed=seed, name=name, norm=norm, k=k, eta=eta, loss=loss, opt=opt, sides=sides, n_ent=n_ent, n_rel=n_rel, n=n,
                bc=bc, epochs=epochs, lr=lr, X=X, ent0=ent0, rel0=rel0, emp=emp, reg=reg, reg_kw=reg_kw, kw=kw,
                omodel=("TransE_L%d" % norm) if name == "TransE" else name,
                what=str((name, norm, k, eta, loss, opt, sides, n_ent, n_rel, n, bc, epochs, lr, reg)))


def _state_arrays(tr):
    """the optimizer state of both tables under the oracle's names (unpadded host copies)"""
    names = {"momentum": ("m",), "adagrad": ("acc",), "adam": ("m", "v")}.get(tr.opt_name, ())
    out = {}
    for tbl, st in (("E", tr.state_ent), ("R", tr.state_rel)):
        out[tbl] = {nm: np.ascontiguousarray(st[i].cpu().numpy()) for i, nm in enumerate(names)}
    return out


def record_steps(monkeypatch):
    """patch Trainer.run_batches (see the module's docstring); returns the list the snapshots go to, [0] = before the first step"""
    from emgraph_amd.training import Trainer
    snaps = []

    def snap(tr, spec, loss):
        E, R = tr.tables_numpy()
        snaps.append({"spec": spec, "E": E, "R": R, "state": _state_arrays(tr), "step": tr.step_count, "loss": loss})

    def run_batches(self, specs):
        specs = [s for s in specs if s is not None and s[1] > 0]
        prev = self.read_loss(reset=False)
        if not snaps:
            snap(self, None, 0.0)
        for i, s in enumerate(specs):
            self.step(s[0], s[1], epoch=s[2], batch=s[3], n_choices=s[4] if len(s) > 4 else None,
                      entities_list=s[5] if len(s) > 5 else None, prefetch=specs[i + 1:i + 4])
            cum = self.read_loss(reset=False)
            snap(self, tuple(int(v) for v in s[:4]), cum - prev)
            prev = cum

    monkeypatch.setattr(Trainer, "run_batches", run_batches)
    return snaps


def _ulp(x):
    return np.spacing(np.abs(x.astype(F32))).astype(np.float64)


def _fit(cfg):
    from emgraph_amd import models
    m = getattr(models, cfg["name"])(**cfg["kw"])
    try:
        m.fit(cfg["X"])
    except ValueError as e:
        assert "Loss is" in str(e), (cfg["what"], str(e))
        return m, str(e)
    return m, None


def check_step_by_step(cfg, monkeypatch, stats=None):
    """the step-by-step soak of one configuration (see the module's docstring).  Returns a dict: steps checked, elements within
    rounding of a jump (J > 0: 'exempt') and elements the jump allowance was needed for ('excused') over all steps, the largest
    observed / allowed ratio (elements with J = 0, error past the last 2 ulps over the interval's half width), whether the run
    stopped with a non-finite loss."""
    import torch  # noqa: F401

    what = cfg["what"]
    with monkeypatch.context() as mp:
        snaps = record_steps(mp)
        m1, err1 = _fit(cfg)
    m2, err2 = _fit(cfg)          # the default path: graph replays where the shape allows them
    assert (err1 is None) == (err2 is None), (what, err1, err2)
    if err1 is None:
        np.testing.assert_array_equal(m1.trained_model_params[0], m2.trained_model_params[0], err_msg=what)
        np.testing.assert_array_equal(m1.trained_model_params[1], m2.trained_model_params[1], err_msg=what)
        np.testing.assert_allclose(m1.epoch_losses, m2.epoch_losses, rtol=1e-8 if cfg["reg"] is not None else 1e-12, err_msg=what)
    else:
        assert err1 == err2, (what, err1, err2)

    X = cfg["X"].astype(np.int32)
    opt, lr, reg, sides, eta, k = cfg["opt"], cfg["lr"], cfg["reg"], cfg["sides"], cfg["eta"], cfg["k"]
    n_ent = cfg["n_ent"]
    out = {"steps": 0, "exempt": 0, "excused": 0, "ratio": 0.0, "diverged": err1 is not None}
    np.testing.assert_array_equal(snaps[0]["E"], cfg["ent0"], err_msg=what)
    np.testing.assert_array_equal(snaps[0]["R"], cfg["rel0"], err_msg=what)
    if err1 is None:              # every optimizer step of the run went through the patched loop: none is left unchecked
        bs = -(-len(X) // cfg["bc"])
        n_steps = cfg["epochs"] * sum(1 for b in range(cfg["bc"]) if b * bs < len(X))
        assert len(snaps) - 1 == n_steps, (what, len(snaps) - 1, n_steps)
    finite = True
    for t in range(1, len(snaps)):
        pre, post = snaps[t - 1], snaps[t]
        if not all(np.all(np.isfinite(a)) for a in (pre["E"], pre["R"], post["E"], post["R"])) or not np.isfinite(post["loss"]):
            finite = False
            break                 # compared for as long as the run stays finite
        assert post["step"] == t, (what, post["step"], t)
        start, B, epoch, batch = post["spec"]
        xb = X[start:start + B]
        x_negs = []
        for sd, side in enumerate(sides):
            counter = ((epoch - 1) * cfg["bc"] + (batch - 1)) * len(sides) + sd
            x_negs.append(orc.generate_corruptions_for_fit_philox(xb, eta=eta, corrupt_side=side, entities_size=n_ent,
                                                                  seed=cfg["seed"], counter=counter))
        with np.errstate(over="ignore", invalid="ignore"):
            bd = orc.train_grads_bounds(cfg["omodel"], pre["E"], pre["R"], xb, eta, cfg["loss"], None, x_negs, k=k, reg=reg)
        where = "%s step %d" % (what, t)
        cnt = bd["counts"]
        n_tch = cnt["touched_E"] + cnt["touched_R"]
        out["exempt"] += cnt["exempt_E"] + cnt["exempt_R"]
        n_used = 0                 # elements only the jump allowance J let through
        # the step's loss (the device's double; the regulariser's value included)
        assert abs(post["loss"] - bd["loss"]) <= bd["loss_allow"], (where, post["loss"], bd["loss"], bd["loss_allow"])
        if bd["loss_allow"] > 0:
            out["ratio"] = max(out["ratio"], abs(post["loss"] - bd["loss"]) / bd["loss_allow"])
        for tbl in "ER":
            W0, W1 = pre[tbl], post[tbl]
            g, d = bd["d" + tbl], bd["A" + tbl] + bd["J" + tbl]
            touched = bd["touched_" + tbl]
            st0 = {nm: a.copy() for nm, a in pre["state"][tbl].items()}
            if opt == "adam":
                st0["t"] = t - 1
            kw = dict(lr=lr, touched=None if opt == "adam" else touched)
            with np.errstate(over="ignore", invalid="ignore"):
                iv = orc.opt_apply_interval(opt, W0, g, d, st0, **kw)
                ivA = orc.opt_apply_interval(opt, W0, g, bd["A" + tbl], st0, **kw)
                pt = orc.opt_apply_interval(opt, W0, g, 0.0, st0, **kw)
            ok_rows = ~bd["exempt_" + tbl]
            used = np.zeros(W0.shape, bool)
            for key, (lo, hi) in iv.items():
                if key == "w" and opt == "adam":
                    continue
                got = W1 if key == "w" else post["state"][tbl][key]
                prev = (W0 if key == "w" else pre["state"][tbl][key]).astype(np.float64)
                # the last roundings of the update: 2 ulps of the result, of the value before, and of the change itself
                last = 2 * (_ulp(prev) + _ulp(pt[key][0].astype(np.float64) - prev))
                inside = lambda lo, hi: (got >= lo.astype(np.float64) - 2 * _ulp(lo) - last) & (got <= hi.astype(np.float64) + 2 * _ulp(hi) + last)  # noqa: E731
                bad = ~inside(lo, hi)
                if bad.any():
                    i = tuple(np.argwhere(bad)[0])
                    raise AssertionError("%s: table %s %s, %d elements outside the interval; first %s: got %r, interval [%r, %r], "
                                         "g %r, A %r, J %r" % (where, tbl, key, int(bad.sum()), i, float(got[i]), float(lo[i]),
                                                               float(hi[i]), g[i], bd["A" + tbl][i], bd["J" + tbl][i]))
                used |= ~inside(*ivA[key])
                lo64, hi64, p0 = lo.astype(np.float64), hi.astype(np.float64), pt[key][0].astype(np.float64)
                allow = np.maximum(hi64 - p0, p0 - lo64)
                err = np.maximum(np.abs(got - p0) - 2 * _ulp(pt[key][0]) - last, 0.0)
                sel = ok_rows & (allow > 0) & np.isfinite(allow)
                if sel.any():
                    out["ratio"] = max(out["ratio"], float((err[sel] / allow[sel]).max()))
            n_used += int(used.sum())
            if opt == "adam":           # the table from the moments the step itself wrote
                m_new, v_new = post["state"][tbl]["m"], post["state"][tbl]["v"]
                want = orc.adam_table_from_state(W0, m_new, v_new, lr, t).astype(np.float64)
                tol = 4 * _ulp(want) + 4 * _ulp(W0.astype(np.float64) - want)
                bad = ~(np.abs(W1 - want) <= tol)
                assert not bad.any(), (where, tbl, "Adam's table", int(bad.sum()), np.argwhere(bad)[0])
            # rows the oracle leaves alone: the same bits
            if reg is None:
                if opt == "adam":
                    still = ~touched & np.all(pre["state"][tbl]["m"] == 0, 1) & np.all(pre["state"][tbl]["v"] == 0, 1)
                else:
                    still = ~touched
                np.testing.assert_array_equal(W1[still], W0[still], err_msg=where + " untouched rows of " + tbl)
                for key, a in post["state"][tbl].items():
                    np.testing.assert_array_equal(a[still], pre["state"][tbl][key][still], err_msg=where + " state " + key)
        # an element is excused by a jump only where the jump allowance was needed: at most 1 % of the touched ones
        assert n_used <= 0.01 * n_tch, (where, "%d elements excused by a jump of %d touched (%d within rounding of one)"
                                        % (n_used, n_tch, cnt["exempt_E"] + cnt["exempt_R"]))
        out["excused"] += n_used
        out["steps"] += 1
    assert out["steps"] == len(snaps) - 1 or not finite, (what, out["steps"], len(snaps) - 1)
    assert out["steps"] > 0 or err1 is not None, (what, "no step checked")
    if stats is not None:
        stats.update(out)
    return out
