"""The default calibration without negatives at the evaluation shape: ComplEx k=200, |E| = 1M random-normal tables, 1e5
positives, batches_count=100 x epochs=50 = 5000 optimiser steps of 1000 rows.  Times (1) the fused path (emg_calib_step: one
launch per step, the state record read once at the end) and (2) the same steps composed from the existing entry points —
emg_corrupt_fit + emg_score_triples per step, the scores read by the host, the weighted loss gradient and Keras Adam in
float64 numpy — and checks that both end at the same (w, b).  Wall clock around a device synchronisation (the composed path
IS host-paced: events on the stream would not see it), one warm-up call, median of 3.  One JSON line."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from emgraph_amd import _lib as L  # noqa: E402
from emgraph_amd import calibration as K  # noqa: E402
from emgraph_amd import device as D  # noqa: E402
from emgraph_amd.training import alloc_table  # noqa: E402

N_ENT, N_REL, KDIM, N_POS = 1_000_000, 1000, 200, 100_000
KI = 2 * KDIM
BATCHES, EPOCHS, RATE, SEED = 100, 50, 0.5, 0
REPS = 3


def composed(ent, rel, x_pos):
    dev = ent.device
    X = torch.from_numpy(x_pos).to(dev)
    sp = D.score_triples(L.COMPLEX, ent, rel, KI, 1.0, X)
    lp, ln, wp, wn, b0 = K.platt_constants(N_POS, N_POS, RATE, 1, 1)
    bs = int(np.ceil(N_POS / BATCHES))
    w, b, m, v, t = 0.0, b0, np.zeros(2), np.zeros(2), 0
    for epoch in range(EPOCHS):
        for i in range(BATCHES):
            xb = X[i * bs:(i + 1) * bs]
            neg = D.corrupt_fit(xb, 1, L.SIDE_SO, entities_size=N_ENT, seed=SEED, counter=epoch * BATCHES + i)
            sn = D.score_triples(L.COMPLEX, ent, rel, KI, 1.0, neg).cpu().numpy().astype(np.float64)
            s_p = sp[i * bs:(i + 1) * bs].cpu().numpy().astype(np.float64)
            g = np.zeros(2)
            for s, z, wt in ((s_p, lp, wp), (sn, ln, wn)):
                x = -(w * s + b)
                e = np.exp(-np.abs(x))
                d = wt * (np.where(x >= 0, 1 / (1 + e), e / (1 + e)) - z)
                g += np.array([np.sum(-d * s), np.sum(-d)])
            g /= len(s_p) + len(sn)
            t += 1
            lr_t = K.ADAM_LR * np.sqrt(1 - K.ADAM_BETA2 ** t) / (1 - K.ADAM_BETA1 ** t)
            m = K.ADAM_BETA1 * m + (1 - K.ADAM_BETA1) * g
            v = K.ADAM_BETA2 * v + (1 - K.ADAM_BETA2) * g * g
            w, b = np.array([w, b]) - lr_t * m / (np.sqrt(v) + K.ADAM_EPS)
    return float(w), float(b)


def timed(fn):
    fn()
    torch.cuda.synchronize()
    secs, out = [], None
    for _ in range(REPS):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
    return statistics.median(secs), secs, out


def main():
    D.require_gpu()
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(1)
    ent = alloc_table(N_ENT, KI, dev, init=torch.randn((N_ENT, KI), generator=g, device=dev) * 0.3)
    rel = alloc_table(N_REL, KI, dev, init=torch.randn((N_REL, KI), generator=g, device=dev) * 0.3)
    rs = np.random.RandomState(2)
    x_pos = np.stack([rs.randint(0, N_ENT, N_POS), rs.randint(0, N_REL, N_POS), rs.randint(0, N_ENT, N_POS)], 1).astype(np.int32)
    fused_s, fused_all, wb_f = timed(lambda: K.calibrate_with_corruptions(L.COMPLEX, ent, rel, KI, 1.0, x_pos, RATE, BATCHES, EPOCHS, SEED))
    comp_s, comp_all, wb_c = timed(lambda: composed(ent, rel, x_pos))
    steps = BATCHES * EPOCHS
    print(json.dumps({"shape": "ComplEx k=200 |E|=1M n_pos=1e5 steps=%d" % steps, "fused_s": fused_s, "fused_us_per_step": 1e6 * fused_s / steps,
                      "composed_s": comp_s, "composed_us_per_step": 1e6 * comp_s / steps, "fused_runs_s": fused_all, "composed_runs_s": comp_all,
                      "w_b_fused": wb_f, "w_b_composed": wb_c,
                      "agree": bool(abs(wb_f[0] - wb_c[0]) <= 1e-6 * max(1, abs(wb_c[0])) and abs(wb_f[1] - wb_c[1]) <= 1e-6 * max(1, abs(wb_c[1])))}))


if __name__ == "__main__":
    main()
