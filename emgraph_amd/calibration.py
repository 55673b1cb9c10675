"""Platt-scaling calibration of a fitted model's scores — the host side of emg_calib.hip (EmbeddingModel.py:2212-2575:
_calibrate_with_corruptions, _calibrate_with_negatives, _calibrate, _predict_proba; AmpliGraph 1.x's calibrate /
predict_proba).  Everything per score happens on the device; here are the labels and weights (:2439-2499), the Newton
iteration of the mode with negatives and the launch loop of the mode without.
"""
from __future__ import annotations

import logging
import math

import numpy as np
import torch

from . import _lib as L
from . import device as D

logger = logging.getLogger(__name__)

# tf.keras.optimizers.Adam() (:2509)
ADAM_LR, ADAM_BETA1, ADAM_BETA2, ADAM_EPS = 1e-3, 0.9, 0.999, 1e-7
NEWTON_MAX_ITER, NEWTON_DECREMENT, NEWTON_RIDGE, NEWTON_MIN_STEP = 100, 1e-20, 1e-12, 2.0 ** -20


def platt_constants(n_pos, n_neg, positive_base_rate, n_pos_scores, n_neg_scores):
    """(label_pos, label_neg, weight_pos, weight_neg, b0): :2443-2454 (Platt's smoothed targets), :2491-2499 (the sample weights
    that make the base rate hold whatever the batch sizes), :2475-2482 (the bias the iteration starts from; w starts at 0)"""
    return ((n_pos + 1.0) / (n_pos + 2.0), 1.0 / (n_neg + 2.0), float(n_neg_scores) / float(n_pos_scores),
            (1.0 - positive_base_rate) / positive_base_rate, math.log((n_neg + 1.0) / (n_pos + 1.0)))


def newton_minimise(moments, w, b):
    """Minimiser of the strictly convex objective whose (loss, g_w, g_b, h_ww, h_wb, h_bb) ``moments(w, b)`` returns: Newton
    steps on the ridged 2 x 2 Hessian, halved while the loss does not decrease, until the Newton decrement is at most 1e-20
    (AmpliGraph: L-BFGS to convergence — no hyper-parameter enters).  The moments of an accepted point are the next
    iteration's: one evaluation per iteration where the full step is taken."""
    m = moments(w, b)
    for _ in range(NEWTON_MAX_ITER):
        g = np.array([m[1], m[2]])
        H = np.array([[m[3] + NEWTON_RIDGE, m[4]], [m[4], m[5] + NEWTON_RIDGE]])
        d = np.linalg.solve(H, g)
        if not float(g @ d) > NEWTON_DECREMENT:
            break
        t = 1.0
        while True:
            cand = (w - t * d[0], b - t * d[1])
            mc = moments(*cand)
            if mc[0] <= m[0]:
                break
            t *= 0.5
            if t < NEWTON_MIN_STEP:
                return w, b
        (w, b), m = cand, mc
    return w, b


def calibrate_with_negatives(model_id, ent, rel, k_int, scale, x_pos, x_neg, positive_base_rate):
    """:2262-2287 + :2421-2424: both sets are scored once; every Newton iteration is one launch and one 48-byte read"""
    dev = ent.device
    sp = D.score_triples(model_id, ent, rel, k_int, scale, torch.from_numpy(x_pos).to(dev))
    sn = D.score_triples(model_id, ent, rel, k_int, scale, torch.from_numpy(x_neg).to(dev))
    n_pos, n_neg = len(x_pos), len(x_neg)
    lp, ln, wp, wn, b0 = platt_constants(n_pos, n_neg, positive_base_rate, n_pos, n_neg)
    ws = D.calib_workspace(n_pos + n_neg, dev)
    out = torch.empty(6, dtype=torch.float64, device=dev)

    def moments(w, b):
        return D.calib_moments(sp, sn, float(w), float(b), lp, ln, wp, wn, out, ws).cpu().numpy()

    return newton_minimise(moments, 0.0, b0)


def calibrate_with_corruptions(model_id, ent, rel, k_int, scale, x_pos, positive_base_rate, batches_count, epochs, seed,
                               verbose=False):
    """:2212-2260 + :2509-2531: epochs x batches_count fused steps (emg_calib_step) on the contiguous slices fit() uses, draw
    counter epoch * batches_count + batch; the device state record is read once at the end (and once per epoch when verbose)"""
    dev = ent.device
    n_pos = len(x_pos)
    X = torch.from_numpy(x_pos).to(dev)
    sp = D.score_triples(model_id, ent, rel, k_int, scale, X)
    lp, ln, wp, wn, b0 = platt_constants(n_pos, n_pos, positive_base_rate, 1, 1)   # a batch scores one negative per positive
    batch_size = int(np.ceil(n_pos / batches_count))
    ws = D.calib_workspace(batch_size, dev)
    state = torch.zeros(8, dtype=torch.float64)
    state[1] = b0
    state = state.to(dev)
    slices = [(i, i * batch_size, min((i + 1) * batch_size, n_pos)) for i in range(batches_count)]
    slices = [(i, X[lo:hi], sp[lo:hi]) for i, lo, hi in slices if hi > lo]   # an empty slice is no step
    loss_seen = 0.0
    for epoch in range(epochs):
        for i, xb, sb in slices:
            D.calib_step(model_id, ent, rel, k_int, scale, xb, sb, seed, epoch * batches_count + i, lp, ln, wp, wn, state, ws,
                         lr=ADAM_LR, beta1=ADAM_BETA1, beta2=ADAM_BETA2, eps=ADAM_EPS)
        if verbose:
            loss_sum = float(state[7].item())
            logger.debug("Calibration Loss: {:10f}".format((loss_sum - loss_seen) / batches_count))   # :2526
            loss_seen = loss_sum
    st = state.cpu().numpy()
    return float(st[0]), float(st[1])


def predict_proba(model_id, ent, rel, k_int, scale, x_idx, w, b, chunk=1 << 22):
    """:2564-2570"""
    out = np.empty(len(x_idx), dtype=np.float32)
    for c0 in range(0, len(x_idx), chunk):
        xt = torch.from_numpy(x_idx[c0:c0 + chunk]).to(ent.device)
        sc = D.score_triples(model_id, ent, rel, k_int, scale, xt)
        out[c0:c0 + chunk] = D.calib_proba(sc, float(w), float(b)).cpu().numpy()
    return out
