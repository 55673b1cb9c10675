"""replay one seed of tests/test_api.py::test_fit_random_configurations_match_oracle_training_loop and say WHERE the fitted tables leave
the oracle's: per epoch count, the rows that differ, how many of their elements, and whether the difference looks like a flipped
sign of TransE-L1's gradient (a coordinate whose difference is within rounding of zero).  usage: python tools/dbg_fuzz_seed.py SEED"""
import os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import test_api as TA
from oracle import emgraph_oracle as orc
F32 = np.float32
seed = int(sys.argv[1])
cfg = TA._random_fit_config(seed)
name, norm, k, eta, loss, opt, sides = (cfg[a] for a in ("name", "norm", "k", "eta", "loss", "opt", "sides"))
bc, epochs, lr, X, ent0, rel0, emp = (cfg[a] for a in ("bc", "epochs", "lr", "X", "ent0", "rel0", "emp"))
reg, reg_kw = cfg["reg"], cfg["reg_kw"]
print("config:", cfg["what"])
omodel = cfg["omodel"]
for ep in range(1, epochs + 1):
    m = TA._models()[name](k=k, eta=eta, epochs=ep, batches_count=bc, seed=seed, loss=loss, optimizer=opt, optimizer_params={"lr": lr},
                           embedding_model_params=emp, initializer="constant", initializer_params={"entity": ent0, "relation": rel0}, **reg_kw)
    m.fit(X)
    E, R, losses = TA.oracle_fit(omodel, k, X.astype(np.int32), ent0, rel0, eta, ep, bc, seed, loss, None, opt, lr, sides=sides, reg=reg)
    G = m.trained_model_params[0]
    bad = ~np.isclose(G, E, rtol=2e-3, atol=2e-5)
    rows = np.nonzero(bad.any(1))[0]
    print("epochs %d: %d elements off in %d rows; losses got %s oracle %s" % (ep, int(bad.sum()), len(rows), [round(float(x), 5) for x in m.epoch_losses], [round(float(x), 5) for x in losses]))
    for r_ in rows[:12]:
        d = G[r_] - E[r_]
        print("   row %d: %d off, max |diff| %.3e, diff values (first 6 off): %s ; in X as s %d, as o %d" % (
            r_, int(bad[r_].sum()), np.abs(d).max(), np.round(d[bad[r_]][:6], 5).tolist(), int((X[:, 0] == r_).sum()), int((X[:, 2] == r_).sum())))
    bR = ~np.isclose(m.trained_model_params[1], R, rtol=2e-3, atol=2e-5)
    print("   relation table: %d elements off" % int(bR.sum()))
