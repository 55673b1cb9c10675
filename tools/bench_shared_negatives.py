"""Training step at the C3 shape (ComplEx k=200 eta=20, |E|=1M |R|=1k, B=16384, NLL, SGD: bench.py's flagship workload, same
triples and tables) with SHARED negatives (Trainer(shared_negatives=C), DESIGN.md 4.1 "Shared negatives") for C in {1, 16, 64},
alternated with the default step (fused, in place, pipelined: what bench.py times) in the same process on the same box: ``--rounds``
timed windows each (default four), default / C = 1 / C = 16 / C = 64 in turn within a round.

Per variant: ms per step of every window, the step's OWN byte count (``step_bytes`` below: the rows a step has to move, from its
shapes and the number of distinct destinations of one prepared batch) and the achieved TB/s against it, and the HIP-event times of
the stages.  The byte count is the algorithm's, not a profile: re-reads served by a cache are not in it.  ``--only`` times one
variant alone in the process (several trainers of this size in one process change each other's timings).

    python tools/bench_shared_negatives.py [--only default|1|16|64] [--steps 1000] [--shared-steps 200] [--warmup 20] [--rounds 4]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402  (the workload table, its triples and its initial tables)

CHUNKS = (1, 16, 64)


def step_bytes(B, eta_total, k_int, n_unique_ent, n_unique_rel, C=None):
    """bytes one SGD step has to move, rows of ``k_int`` floats.  ``C`` = None: the ordinary step (one replacement row per positive and
    slot, scored and differentiated in ONE fused pass); otherwise the shared step's three passes.
      gathered rows  3 B (s, p, o) + the replacement rows: eta_total * B, or eta_total * G shared ones
      forward        (shared: a pass of its own) reads the gathered rows, writes (1 + eta_total) B scores; the loss reads them and
                     writes as many gradients, which the backward reads
      backward       reads the gathered rows, writes one gradient row per gathered row
      apply          reads the gradient rows, reads and writes every distinct destination row once
    (the ordinary step's in-place singletons skip the gradient row's write and read: not credited here, so its figure is an upper
    bound of what it must move)"""
    row = 4 * k_int
    G = -(-B // C) if C else B
    gathered = 3 * B + eta_total * G
    passes = 1 if C is None else 2
    scores = 0 if C is None else 4 * 4 * (1 + eta_total) * B
    return gathered * row * (passes + 2) + scores + 2 * (n_unique_ent + n_unique_rel) * row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000, help="timed steps per window of the default step")
    ap.add_argument("--shared-steps", type=int, default=200, help="timed steps per window of a shared-negatives variant")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--only", default=None, help="default | 1 | 16 | 64: one variant alone in this process")
    args = ap.parse_args()
    names = ["default"] + [str(c) for c in CHUNKS]
    variants = [n for n in names if args.only in (None, n)]
    if not variants:
        ap.error("--only: default | 1 | 16 | 64")
    import torch

    from emgraph_amd.training import Trainer
    w = bench.WORKLOADS["C3"]
    k_int, B, nb, eta = 2 * w["k"], w["B"], bench.N_RESIDENT, w["eta"]
    rs = np.random.RandomState(0)
    ent0, rel0 = bench.glorot(rs, w["n_ent"], k_int), bench.glorot(rs, w["n_rel"], k_int)
    X = bench.make_triples(w, nb * B, 1234)
    runs = {}
    for name in variants:
        kw = {} if name == "default" else {"shared_negatives": int(name)}
        tr = Trainer(bench.MODEL_IDS[w["model"]], k_int, 1.0, ent0, rel0, eta, loss=w["loss"], optimizer=w["optimizer"],
                     optimizer_params={"lr": 0.0005}, batches_count=nb, seed=0, **kw)
        tr.set_training_set(X, B)
        runs[name] = {"tr": tr, "i": 0, "ms": [], "steps": args.steps if name == "default" else args.shared_steps}

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
    out = {"workload": w["desc"], "rounds": args.rounds, "variants": {}}
    for name in variants:
        r = runs[name]
        tr = r["tr"]
        C = None if name == "default" else int(name)
        n_ce = (2 + eta) * B if C is None else 2 * B + eta * (-(-B // C))
        tr.enable_stage_timing(8)
        run(r, 8)
        stages = {k: round(float(np.mean(v)), 4) for k, v in tr.stage_times_ms().items()}
        torch.cuda.synchronize()
        sl = tr.slots[0]        # any slot holds the destinations of a prepared batch of this shape
        n_ue = int(torch.unique(sl["dest_ent"][:n_ce]).numel())
        n_ur = int(torch.unique(sl["dest_rel"][:B]).numel())
        nbytes = step_bytes(B, eta, k_int, n_ue, n_ur, C)
        assert np.isfinite(tr.read_loss())
        ms = sorted(r["ms"])
        med = 0.5 * (ms[(len(ms) - 1) // 2] + ms[len(ms) // 2])
        out["variants"][name] = {"ms_per_step": [round(v, 4) for v in r["ms"]], "ms_median": round(med, 4), "steps_per_window": r["steps"],
                                 "gradient_rows_ent": n_ce, "distinct_dest_ent": n_ue, "distinct_dest_rel": n_ur,
                                 "step_bytes": int(nbytes), "stages_ms": stages,
                                 # (the default step's count is an upper bound — in-place singletons and factored rows move less —: no rate from it)
                                 "achieved_TBps": round(nbytes / (med * 1e-3) / 1e12, 4) if C is not None else None,
                                 "corruption_rows_per_step": tr.negative_sampling_stats()["rows"] // max(1, tr.step_count)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
