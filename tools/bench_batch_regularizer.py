"""Training step at the C3 shape (ComplEx k=200 eta=20, |E|=1M |R|=1k, B=16384, NLL, SGD: bench.py's flagship workload, same
triples and tables) under the batch-local regulariser (Trainer(regularizer='N3'), DESIGN.md 4.1 "Batch regulariser"), alternated in
one process on one box, ``--rounds`` timed windows each (default four), a / b / c / d in turn within a round:

    a   'N3': the host-driven unfused step + emg_batchreg's 3 B gradient rows behind its own
    b   the same host-driven unfused step with no regulariser (Trainer(fused=False, inplace=False, pipeline=False), not factored, with
        its step plan dropped, so that the host issues every launch as it does in a): what a is measured against
    c   'LP': the full-table regulariser folded into the fused step
    d   bench.py's default step (fused, in place, pipelined), untouched: the anchor

Per variant: ms per step of every window and the HIP-event times of the stages.  Then emg_batchreg alone (HIP events around it,
``--kernel-reps`` launches) against its own byte count — 3 rows read and 3 rows written per positive, k_int floats each, plus the ids
and destinations — and that count at the bandwidth the entity apply reaches in b (its stage time against the contribution rows it
reads plus one read and one write of every distinct destination row of the batch).
``--only`` times one variant alone in the process.

    python tools/bench_batch_regularizer.py [--only a|b|c|d] [--steps 1000] [--unfused-steps 200] [--warmup 20] [--rounds 4]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402  (the workload table, its triples and its initial tables)

LAMBDA = 1e-5
VARIANTS = {"a": dict(regularizer="N3", regularizer_params={"lambda": LAMBDA}),
            "b": dict(fused=False, inplace=False, pipeline=False),
            "c": dict(regularizer="LP", regularizer_params={"lambda": LAMBDA, "p": 3}),
            "d": dict()}


def drop_plan(tr):
    """the host issues every launch of the step (the shape of Trainer._compute_batchreg) instead of one emg_plan_step"""
    from emgraph_amd import _lib as L
    if tr.plan is not None:
        L.check(L.load().emg_plan_destroy(tr.plan), "emg_plan_destroy")
        tr.plan = None
    tr.graph = False


def time_kernel(tr, B, k_int, reps):
    import torch
    from emgraph_amd import _lib as L
    from emgraph_amd import device as D
    pos = tr.X[:B]
    ldc = tr.contrib_ent.stride(0)
    ce = torch.empty((2 * B, ldc), dtype=torch.float32, device=tr.device)[:, :k_int]
    cr = torch.empty((B, ldc), dtype=torch.float32, device=tr.device)[:, :k_int]
    de, dr = torch.empty(2 * B, dtype=torch.int32, device=tr.device), torch.empty(B, dtype=torch.int32, device=tr.device)
    val = torch.zeros(1, dtype=torch.float64, device=tr.device)
    fn = lambda: D.batch_reg(tr.ent, tr.rel, k_int, pos, 3, LAMBDA, LAMBDA, L.BATCHREG_MODULUS, L.BATCHREG_MODULUS, ce, de, cr, dr,  # noqa: E731
                             value=val)
    fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    med = ms[len(ms) // 2]
    nbytes = 6 * B * 4 * k_int + 4 * 3 * B * 2
    return {"ms_min": round(ms[0], 4), "ms_median": round(med, 4), "ms_max": round(ms[-1], 4), "bytes": int(nbytes),
            "TBps_at_median": round(nbytes / (med * 1e-3) / 1e12, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000, help="timed steps per window of the fused steps (c, d)")
    ap.add_argument("--unfused-steps", type=int, default=200, help="timed steps per window of variants a, b")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--only", default=None, help="a | b | c | d: one variant alone in this process")
    args = ap.parse_args()
    variants = [n for n in VARIANTS if args.only in (None, n)]
    if not variants:
        ap.error("--only: a | b | c | d")
    import torch

    from emgraph_amd.training import Trainer
    w = bench.WORKLOADS["C3"]
    k_int, B, nb, eta = 2 * w["k"], w["B"], bench.N_RESIDENT, w["eta"]
    rs = np.random.RandomState(0)
    ent0, rel0 = bench.glorot(rs, w["n_ent"], k_int), bench.glorot(rs, w["n_rel"], k_int)
    X = bench.make_triples(w, nb * B, 1234)
    runs = {}
    for name in variants:
        tr = Trainer(bench.MODEL_IDS[w["model"]], k_int, 1.0, ent0, rel0, eta, loss=w["loss"], optimizer=w["optimizer"],
                     optimizer_params={"lr": 0.0005}, batches_count=nb, seed=0, **VARIANTS[name])
        if name == "b":
            tr.factored = False      # every negative's gradient row written out, as a's step writes them
        tr.set_training_set(X, B)
        if name == "b":
            drop_plan(tr)
        runs[name] = {"tr": tr, "i": 0, "ms": [], "steps": args.steps if name in ("c", "d") else args.unfused_steps}

    def spec(i):
        return ((i % nb) * B, B, i // nb + 1, i % nb + 1)

    def run(r, n):
        for _ in range(n):
            i = r["i"]
            s = spec(i)
            r["tr"].step(s[0], s[1], epoch=s[2], batch=s[3], prefetch=[spec(i + 1), spec(i + 2), spec(i + 3)])
            r["i"] += 1

    for r in runs.values():
        run(r, args.warmup)
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name in variants:
            r = runs[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(r, r["steps"])
            torch.cuda.synchronize()
            r["ms"].append((time.perf_counter() - t0) / r["steps"] * 1e3)
    out = {"workload": w["desc"], "rounds": args.rounds, "lambda": LAMBDA, "variants": {}}
    for name in variants:
        r = runs[name]
        tr = r["tr"]
        tr.enable_stage_timing(8)
        run(r, 8)
        stages = {k: round(float(np.mean(v)), 4) for k, v in tr.stage_times_ms().items()}
        torch.cuda.synchronize()
        assert np.isfinite(tr.read_loss())
        ms = sorted(r["ms"])
        out["variants"][name] = {"regularizer": VARIANTS[name].get("regularizer"), "fused": bool(tr.fused), "plan": tr.plan is not None,
                                 "ms_per_step": [round(v, 4) for v in r["ms"]], "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4),
                                 "steps_per_window": r["steps"], "stages_ms": stages}
    if "a" in runs:
        kern = time_kernel(runs["a"]["tr"], B, k_int, args.kernel_reps)
        if "b" in runs and "apply_ent" in out["variants"]["b"]["stages_ms"]:
            # what the entity apply of b moves: its (2 + eta) B contribution rows read, every distinct destination row read and written
            tr = runs["b"]["tr"]
            n_ce = (2 + eta) * B
            distinct = int(torch.unique(tr.slots[0]["dest_ent"][:n_ce]).numel())
            apply_bytes = (n_ce + 2 * distinct) * 4 * k_int
            apply_tbps = apply_bytes / (out["variants"]["b"]["stages_ms"]["apply_ent"] * 1e-3) / 1e12
            kern["apply_ent_TBps"] = round(apply_tbps, 3)
            kern["ms_at_apply_bandwidth"] = round(kern["bytes"] / (apply_tbps * 1e12) * 1e3, 4)
            kern["share_of_that_bandwidth"] = round(kern["ms_at_apply_bandwidth"] / kern["ms_median"], 3)
        out["kernel"] = kern
    print(json.dumps(out))


if __name__ == "__main__":
    main()
