"""Float64 numpy restatement of the calibration semantics (Platt scaling, AmpliGraph 1.x's calibrate; the reference's
EmbeddingModel.py:2439-2531) for tests/test_calibration*.py.  Scores and negatives are INPUTS: nothing here gathers, scores or
draws.

    logit   x = -(w s + b)
    labels  positive (n_pos + 1) / (n_pos + 2), negative 1 / (n_neg + 2);  start w = 0, b = log((n_neg + 1) / (n_pos + 1))
    weights positive #negative scores / #positive scores (of the batch), negative (1 - rate) / rate
    loss    sum weight * ce(label, x) / #scores,  ce(z, x) = max(x, 0) - x z + log1p(exp(-|x|))
"""
import numpy as np


def labels(n_pos, n_neg):
    return (n_pos + 1.0) / (n_pos + 2.0), 1.0 / (n_neg + 2.0)


def start(n_pos, n_neg):
    return 0.0, float(np.log((n_neg + 1.0) / (n_pos + 1.0)))


def weights(rate, n_pos_scores, n_neg_scores):
    return float(n_neg_scores) / float(n_pos_scores), (1.0 - rate) / rate


def ce(z, x):
    return np.maximum(x, 0.0) - x * z + np.log1p(np.exp(-np.abs(x)))


def _sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def moments(sp, sn, w, b, label_pos, label_neg, weight_pos, weight_neg):
    """[loss, dL/dw, dL/db, d2L/dw2, d2L/dwdb, d2L/db2] over the scores sp (positives) and sn (negatives), float64"""
    s = np.concatenate([np.asarray(sp, np.float64), np.asarray(sn, np.float64)])
    z = np.concatenate([np.full(len(sp), label_pos), np.full(len(sn), label_neg)])
    wt = np.concatenate([np.full(len(sp), weight_pos), np.full(len(sn), weight_neg)])
    x = -(w * s + b)
    sig = _sigmoid(x)
    d = wt * (sig - z)            # dL/dx per score; dx/dw = -s, dx/db = -1
    e = np.exp(-np.abs(x))
    h = wt * e / ((1.0 + e) * (1.0 + e))   # sig (1 - sig) without the cancellation of 1 - sig at large x
    n = float(len(s))
    return np.array([np.sum(wt * ce(z, x)), np.sum(-d * s), np.sum(-d), np.sum(h * s * s), np.sum(h * s), np.sum(h)]) / n


def newton(sp, sn, n_pos, n_neg, rate, max_iter=100, decrement=1e-20, ridge=1e-12):
    """minimiser (w, b) of the objective over all scores: Newton on the ridged Hessian, steps halved while the loss does not
    decrease, until g' H^-1 g <= decrement or max_iter iterations"""
    lp, ln = labels(n_pos, n_neg)
    wp, wn = weights(rate, len(sp), len(sn))
    w, b = start(n_pos, n_neg)
    m = moments(sp, sn, w, b, lp, ln, wp, wn)
    for _ in range(max_iter):
        g = m[1:3]
        H = np.array([[m[3] + ridge, m[4]], [m[4], m[5] + ridge]])
        d = np.linalg.solve(H, g)
        if not g @ d > decrement:
            break
        t = 1.0
        while True:
            cw, cb = w - t * d[0], b - t * d[1]
            mc = moments(sp, sn, cw, cb, lp, ln, wp, wn)
            if mc[0] <= m[0]:
                break
            t *= 0.5
            if t < 2.0 ** -20:
                return w, b
        w, b, m = cw, cb, mc
    return w, b


def adam(batches, n_pos, n_neg, rate, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-7):
    """Keras Adam, step by step, over ``batches`` = [(positive scores, negative scores of the step's corruptions), ...] in
    the order of the steps.  Returns the state record [w, b, m_w, m_b, v_w, v_b, step, loss_sum]."""
    lp, ln = labels(n_pos, n_neg)
    w, b = start(n_pos, n_neg)
    m = np.zeros(2)
    v = np.zeros(2)
    loss_sum = 0.0
    t = 0
    for sp, sn in batches:
        wp, wn = weights(rate, len(sp), len(sn))
        mom = moments(sp, sn, w, b, lp, ln, wp, wn)
        g = mom[1:3]
        t += 1
        lr_t = lr * np.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)
        m = beta1 * m + (1.0 - beta1) * g
        v = beta2 * v + (1.0 - beta2) * g * g
        w, b = np.array([w, b]) - lr_t * m / (np.sqrt(v) + eps)
        loss_sum += mom[0]
    return np.array([w, b, m[0], m[1], v[0], v[1], float(t), loss_sum])
