"""FocusE edge weights and score links: a float64 numpy restatement of what the reference does with them
(line numbers: emgraph/models/EmbeddingModel.py), driven by the device's own Philox draws the way tests/_fit_steps.py
drives the oracle.  The oracle's score functions, losses and optimizer rule are used as they are.
"""
import numpy as np

from oracle import emgraph_oracle as orc

F32 = np.float32
LINKS = ("linear", "tanh", "sigmoid", "softplus")


def custom_softplus(x):
    """:90-96 — value log(1 + 9999 e^x) and the gradient the reference defines for it, 1 - 1 / (1 + 9999 e^x)"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore"):
        e = 9999 * np.exp(x)
        return np.log(1 + e), 1 - 1 / (1 + e)


def link(name, x):
    """:679-690 (positives), :801-810 (negatives), :2135-2145 (predict): (phi(x), phi'(x)), the derivative in the form TF's
    gradient of the op takes (tanh: 1 - y^2, sigmoid: y (1 - y), from the output y)"""
    x = np.asarray(x, dtype=np.float64)
    if name == "linear":
        return x, np.ones_like(x)
    if name == "tanh":
        y = np.tanh(x)
        return y, 1 - y * y
    if name == "sigmoid":
        y = 1 / (1 + np.exp(-x))
        return y, y * (1 - y)
    if name == "softplus":
        return custom_softplus(x)
    raise ValueError("Invalid non-linearity")


def structure_weight(epoch, stop_epoch=251, structural_wt=0.001):
    """:692-714, with the training loop's 1-based epoch (the feed_dict of :1391 the TF2 port left commented out)"""
    assert stop_epoch >= 0, "Invalid value for stop_epoch"
    if stop_epoch == 0:
        assert 0 <= structural_wt <= 1, "Invalid structure_weight passed to model params!"
        return float(structural_wt)
    return max(1 - epoch / stop_epoch, 0.001)


def weights(w, sw):
    """:716-722 — (weight of the positives, weight of each positive's negatives); w [B] or None (no FocusE: ones)"""
    if w is None:
        return None, None
    w = np.asarray(w, dtype=np.float64)
    return sw + (1 - sw) * (1 - w), sw + (1 - sw) * w


def normalize_literal(X, values, normalize_numeric_values=True):
    """:1181-1228 transcribed statement by statement (the per-relation, per-column normalisation of fit()); works on and
    returns a copy, 2-D"""
    v = np.array(values, dtype=np.float64, copy=True)
    if v.ndim == 1:
        v = v.reshape(-1, 1)
    unique_relations = np.unique(X[:, 1])
    for reln in unique_relations:
        for col_idx in range(v.shape[1]):
            if np.sum(np.isnan(v[X[:, 1] == reln, col_idx])) != v[X[:, 1] == reln, col_idx].shape[0]:
                min_val = np.nanmin(v[X[:, 1] == reln, col_idx])
                max_val = np.nanmax(v[X[:, 1] == reln, col_idx])
                if min_val == max_val:
                    v[X[:, 1] == reln, col_idx] = 1.0
                    continue
                if normalize_numeric_values or min_val < 0 or max_val > 1:
                    v[X[:, 1] == reln, col_idx] = (v[X[:, 1] == reln, col_idx] - min_val) / (max_val - min_val)
            else:
                pass  # all the weights are nans
    return v


def negatives(xb, eta, sides, n_ent, seed, epoch, batch, batches_count):
    """the corruptions fit() draws for batch (epoch, batch), one array per side (the device's Philox counters)"""
    out = []
    for sd, side in enumerate(sides):
        counter = ((epoch - 1) * batches_count + (batch - 1)) * len(sides) + sd
        out.append(orc.generate_corruptions_for_fit_philox(xb, eta=eta, corrupt_side=side, entities_size=n_ent, seed=seed,
                                                           counter=counter))
    return out


def step_terms(model, E, R, xb, eta, loss, loss_params, x_negs, link_name="linear", w=None, sw=1.0, k=None):
    """One batch (:675-816): raw scores -> link -> FocusE weights -> loss; the chain rule back to the raw scores -> table
    gradients.  Returns dict(loss, dE, dR float64, pos, negs raw scores, eff_pos, eff_negs, g_pos, g_negs = dL/d raw score)."""
    E64, R64 = E.astype(np.float64), R.astype(np.float64)
    w_pos, w_neg = weights(w, sw)
    pos = orc.score_triples(model, E64, R64, xb, k=k).astype(np.float64)
    y, dy = link(link_name, pos)
    f_pos = dy if w_pos is None else w_pos * dy
    eff_pos = y if w_pos is None else w_pos * y                                     # :722
    dE, dR = np.zeros(E.shape, np.float64), np.zeros(R.shape, np.float64)
    total, negs, eff_negs, g_negs = 0.0, [], [], []
    g_pos = np.zeros(len(xb), np.float64)
    for x_neg in x_negs:
        neg = orc.score_triples(model, E64, R64, x_neg, k=k).astype(np.float64)
        yn, dyn = link(link_name, neg)
        wn = None if w_neg is None else np.tile(w_neg, eta)                         # :718-720: tiled eta times
        eff_neg = yn if wn is None else wn * yn                                     # :812-813
        f_neg = dyn if wn is None else wn * dyn
        pos_in = np.tile(eff_pos, eta) if orc.REQUIRE_SAME_SIZE[loss] else eff_pos  # :724-729
        with np.errstate(over="ignore"):
            total += float(orc.loss_apply(loss, pos_in, eff_neg, eta, loss_params))  # :816
        gp, gn = orc.loss_grads(loss, eff_pos, eff_neg, eta, loss_params)
        gp, gn = gp.astype(np.float64) * f_pos, gn.astype(np.float64) * f_neg
        g_pos += gp
        for xx, gg in ((xb, gp), (x_neg, gn)):
            a, b = orc.score_grads(model, E64, R64, xx, gg, k=k)
            dE += a
            dR += b
        negs.append(neg)
        eff_negs.append(eff_neg)
        g_negs.append(gn)
    return dict(loss=total, dE=dE, dR=dR, pos=pos, negs=negs, eff_pos=eff_pos, eff_negs=eff_negs, g_pos=g_pos, g_negs=g_negs)


def hinge_gap(loss, terms, loss_params=None):
    """distance of the nearest pair to a kink of the loss (inf where the loss has none): a batch closer than float32 rounding to
    one may take either gradient"""
    margin = (loss_params or {}).get("margin", 1.0)
    gaps = [np.inf]
    for eff_neg in terms["eff_negs"]:
        eta = len(eff_neg) // len(terms["eff_pos"])
        if loss == "pairwise":
            gaps.append(np.abs(margin - np.tile(terms["eff_pos"], eta) + eff_neg).min())
        elif loss == "absolute_margin":
            gaps.append(np.abs(margin + eff_neg).min())
    return float(min(gaps))


def fit_loop(model, E0, R0, X, w, eta, loss, opt, lr, epochs, batches_count, sides, seed, link_name="linear", stop_epoch=251,
             structural_wt=0.001, k=None):
    """fit()'s loop (:1388-1440) on the mapped triples X with the FocusE weights w [n] (or None): per epoch the structure
    weight, per batch step_terms + the optimizer.  Returns (E, R, [epoch loss sums])."""
    E, R = E0.astype(F32).copy(), R0.astype(F32).copy()
    stE, stR = orc.opt_init(opt, E.shape), orc.opt_init(opt, R.shape)
    n = len(X)
    bs = -(-n // batches_count)
    losses = []
    for epoch in range(1, epochs + 1):
        sw = structure_weight(epoch, stop_epoch, structural_wt) if w is not None else 1.0
        tot = 0.0
        for batch in range(1, batches_count + 1):
            xb = X[(batch - 1) * bs:batch * bs]
            if not len(xb):
                continue
            wb = None if w is None else w[(batch - 1) * bs:batch * bs]
            x_negs = negatives(xb, eta, sides, E.shape[0], seed, epoch, batch, batches_count)
            t = step_terms(model, E, R, xb, eta, loss, None, x_negs, link_name, wb, sw, k=k)
            tot += t["loss"]
            tE, tR = np.zeros(E.shape[0], bool), np.zeros(R.shape[0], bool)
            for xx in [xb] + x_negs:
                tE[xx[:, 0]] = True
                tE[xx[:, 2]] = True
            tR[xb[:, 1]] = True
            E = orc.opt_apply(opt, E, t["dE"], stE, lr=lr, touched=None if opt == "adam" else tE)
            R = orc.opt_apply(opt, R, t["dR"], stR, lr=lr, touched=None if opt == "adam" else tR)
        losses.append(tot)
    return E, R, losses
