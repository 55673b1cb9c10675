"""Training step at the C3 shape (ComplEx k=200 eta=20, |E|=1M |R|=1k, B=16384, NLL, SGD: bench.py's flagship workload, same
triples and tables) with RELATION negatives (Trainer(corrupt_sides=[..., 'p']), DESIGN.md 4.1 "Relation negatives"), alternated in
one process on one box, ``--rounds`` timed windows each (default four), a / b / c / d in turn within a round:

    a   bench.py's default step (fused, in place, pipelined), untouched: the anchor
    b   the unfused step with ['s,o'] (Trainer(fused=False)): forward, loss and backward as separate launches
    c   ['s,o', 'p']: b's launches on the entity block + emg_relneg_forward / emg_relneg_backward + a larger grouping and apply
    d   ['p']

Per variant: ms per step of every window and the HIP-event times of the stages.  Then the two new launches alone (HIP events around
each, ``--kernel-reps`` launches) against their OWN byte counts (rows of k_int floats; the relation table is small and stays in L2,
its rows are counted as L2 reads):
    forward    reads 2 entity rows + eta relation rows per positive, writes eta (+ 1) scores
    backward   reads the same, writes eta * B relation rows (+ B with g_pos) and 2 B entity rows
``--only`` times one variant alone in the process.

    python tools/bench_relation_negatives.py [--only a|b|c|d] [--steps 1000] [--unfused-steps 200] [--warmup 20] [--rounds 4]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402  (the workload table, its triples and its initial tables)

VARIANTS = {"a": dict(), "b": dict(fused=False), "c": dict(corrupt_sides=["s,o", "p"]), "d": dict(corrupt_sides=["p"])}


def kernel_bytes(B, eta, k_int, with_pos):
    row = 4 * k_int
    reads = (2 + eta + (1 if with_pos else 0)) * B * row
    fwd = reads + 4 * (eta + (1 if with_pos else 0)) * B + 4 * eta * B
    bwd = reads + ((eta + (1 if with_pos else 0)) * B + 2 * B) * row + 4 * 2 * eta * B
    return fwd, bwd


def time_kernels(tr, B, eta, k_int, reps):
    """HIP-event time of each new launch alone, on the trainer's tables and one batch's codes (both forms: beside entity sides —
    no positives — and alone)"""
    import torch
    from emgraph_amd import device as D
    pos = tr.X[:B]
    codes = D.corrupt_codes(B, eta, 0, tr.n_rel - 1, tr.device, seed=1, counter=1)
    g = torch.full((B * eta,), 0.01, dtype=torch.float32, device=tr.device)
    gp = torch.full((B,), -0.01, dtype=torch.float32, device=tr.device)
    sp = torch.empty(B, dtype=torch.float32, device=tr.device)
    sn = torch.empty(B * eta, dtype=torch.float32, device=tr.device)
    ldc = tr.contrib_ent.stride(0)
    ce = torch.empty((2 * B, ldc), dtype=torch.float32, device=tr.device)[:, :k_int]
    cr = torch.empty(((1 + eta) * B, ldc), dtype=torch.float32, device=tr.device)[:, :k_int]
    de = torch.empty(2 * B, dtype=torch.int32, device=tr.device)
    dr = torch.empty((1 + eta) * B, dtype=torch.int32, device=tr.device)
    out = {}
    for with_pos in (False, True):
        n_cr = (B if with_pos else 0) + eta * B
        fwd = lambda: D.relneg_forward(tr.model_id, tr.ent, tr.rel, k_int, tr.scale, pos, eta, codes,  # noqa: E731
                                       scores_pos=sp if with_pos else None, scores_neg=sn, want_pos=False)
        bwd = lambda: D.relneg_backward(tr.model_id, tr.ent, tr.rel, k_int, tr.scale, pos, eta, codes, gp if with_pos else None, g,  # noqa: E731
                                        ce, cr[:n_cr], de, dr[:n_cr])
        fb, bb = kernel_bytes(B, eta, k_int, with_pos)
        for name, fn, nbytes in (("forward", fwd, fb), ("backward", bwd, bb)):
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
            out[name + ("_with_pos" if with_pos else "")] = {"ms_min": round(ms[0], 4), "ms_median": round(med, 4), "ms_max": round(ms[-1], 4),
                                                             "bytes": int(nbytes), "TBps_at_median": round(nbytes / (med * 1e-3) / 1e12, 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000, help="timed steps per window of the default step")
    ap.add_argument("--unfused-steps", type=int, default=200, help="timed steps per window of variants b, c, d")
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
        tr.set_training_set(X, B)
        runs[name] = {"tr": tr, "i": 0, "ms": [], "steps": args.steps if name == "a" else args.unfused_steps}

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
        tr.enable_stage_timing(8)
        run(r, 8)
        stages = {k: round(float(np.mean(v)), 4) for k, v in tr.stage_times_ms().items()}
        torch.cuda.synchronize()
        assert np.isfinite(tr.read_loss())
        ms = sorted(r["ms"])
        out["variants"][name] = {"sides": VARIANTS[name].get("corrupt_sides", ["s,o"]), "fused": bool(tr.fused),
                                 "ms_per_step": [round(v, 4) for v in r["ms"]], "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4),
                                 "steps_per_window": r["steps"], "stages_ms": stages,
                                 "corruption_rows_per_step": tr.negative_sampling_stats()["rows"] // max(1, tr.step_count)}
    if "c" in runs or "d" in runs:
        out["kernels"] = time_kernels(runs["c" if "c" in runs else "d"]["tr"], B, eta, k_int, args.kernel_reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
