"""Training step at the C3 shape (ComplEx k=200 eta=20, |E|=1M |R|=1k, B=16384, NLL, SGD: bench.py's flagship workload, same
triples and tables) under the negative samplers: uniform (the plain draw), bernoulli, filter, both, and — typed negatives, the pools
being the domains and ranges observed in the workload's triples — typed and typed+filter.  Per variant: ms per
step of every round, the share of redrawn rows and of rows left known, and the HIP-event times of the preparation, scoring and
apply stages.  The filter's known set is the workload's own 1M resident triples.  Time ONE variant per process (``--only``) and
alternate the processes: without it the four trainers share the process, alternate within each round, and change each other's
timings.

    python tools/negative_sampling_throughput.py [--only uniform|bernoulli|filter|both|typed|typed+filter] [--steps 2000] [--warmup 50]
                                                 [--rounds 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402  (the workload table, its triples and its initial tables)

VARIANTS = (("uniform", "uniform", False), ("bernoulli", "bernoulli", False), ("filter", "uniform", True), ("both", "bernoulli", True),
            ("typed", "uniform", False), ("typed+filter", "uniform", True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--retries", type=int, default=4)
    ap.add_argument("--only", default=None, help="one variant alone in this process (uniform | bernoulli | filter | both | typed | typed+filter): several "
                                                 "trainers of this size in one process change each other's timings")
    args = ap.parse_args()
    variants = [v for v in VARIANTS if args.only in (None, v[0])]
    if not variants:
        ap.error("--only: uniform | bernoulli | filter | both | typed | typed+filter")
    import torch

    from emgraph_amd import negative_sampling as NS
    from emgraph_amd.training import Trainer
    w = bench.WORKLOADS["C3"]
    k_int, B, nb = 2 * w["k"], w["B"], bench.N_RESIDENT
    rs = np.random.RandomState(0)
    ent0, rel0 = bench.glorot(rs, w["n_ent"], k_int), bench.glorot(rs, w["n_rel"], k_int)
    X = bench.make_triples(w, nb * B, 1234)
    thr = NS.bernoulli_thresholds(X, w["n_rel"])
    keys = NS.known_triple_keys(X, w["n_ent"], w["n_rel"])
    runs = {}
    for name, side, flt in variants:
        sampler = None
        typed = name.startswith("typed")
        if side == "bernoulli" or flt or typed:
            sampler = {"keep_thr": thr if side == "bernoulli" else None, "known_keys": keys if flt else None, "retries": args.retries}
        if typed:
            from emgraph_amd.type_constraints import TypeConstraints
            sampler["type_constraints"] = TypeConstraints.from_triples(X, (w["n_ent"], w["n_rel"]), from_idx=True)
        tr = Trainer(bench.MODEL_IDS[w["model"]], k_int, 1.0, ent0, rel0, w["eta"], loss=w["loss"], optimizer=w["optimizer"],
                     optimizer_params={"lr": 0.0005}, batches_count=nb, seed=0, negative_sampler=sampler)
        tr.set_training_set(X, B)
        runs[name] = {"tr": tr, "i": 0, "ms": []}

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
        for name, _, _ in variants:
            r = runs[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(r, args.steps)
            torch.cuda.synchronize()
            r["ms"].append((time.perf_counter() - t0) / args.steps * 1e3)
    out = {"workload": w["desc"], "steps": args.steps, "rounds": args.rounds, "known_keys": int(len(keys)), "retries": args.retries,
           "variants": {}}
    for name, _, _ in variants:
        r = runs[name]
        st = r["tr"].negative_sampling_stats()
        r["tr"].enable_stage_timing(16)
        run(r, 16)
        stages = {k: float(np.mean(v)) for k, v in r["tr"].stage_times_ms().items()}
        assert np.isfinite(r["tr"].read_loss())
        out["variants"][name] = {"ms_per_step": [round(v, 4) for v in r["ms"]], "stats": st,
                                 "redrawn_share": st["redrawn"] / max(1, st["rows"]), "known_left_share": st["known_left"] / max(1, st["rows"]),
                                 "prepare_ms": stages.get("prepare"), "fused_ms": stages.get("fused"), "apply_ms": stages.get("apply_ent")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
