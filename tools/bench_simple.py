#!/usr/bin/env python
"""SimplE next to its nearest yardsticks, same device, same run.

Ranking: 8192 test triples x 1M entities, k = 200 (k_int = 400), object side, rank_triples_device at precision 2 (the exact-fast
default) and precision 0 (the exact f32 MFMA kernel) — SimplE next to ComplEx, alternating, --reps times each, on random tables
(N(0, sigma)) and on trained-like ones (every test triple's object aligned with its query vector: tools/bench_link_ranking.py's).
The kernels are the same ones on the same widths; per call the wall time (evaluate level: query rows, half copies of the query
rows, prefilter, re-scoring, counters read back) and the kernels' own time (stats['count_ms'], device events) are printed as
best and worst of the repetitions, with the undecided fraction of precision 2.
Training: the C3 shape (B = 16384, eta = 20, |E| = 1M, |R| = 1000, k_int = 400, nll, SGD), ms per step of the Trainer — SimplE
(generic step) next to RotatE (generic step) and ComplEx (fused step); alternating rounds, best and worst round.

    python tools/bench_simple.py [--n-ent 1000000] [--nq 8192] [--k 200] [--sigma 0.1] [--reps 4] [--steps 20] [--skip-train] [--skip-rank]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from emgraph_amd import _lib as L  # noqa: E402
from emgraph_amd import device as D  # noqa: E402
from emgraph_amd.evaluation.ranking import derived_tables, rank_triples_device  # noqa: E402
from emgraph_amd.training import Trainer, alloc_table  # noqa: E402

RANK_MODELS = (("SimplE", L.SIMPLE, 0.5), ("ComplEx", L.COMPLEX, 1.0))


def rank_tables(mid, scale, a, kind, T):
    ki = 2 * a.k
    g = torch.Generator(device="cuda").manual_seed(0)
    ent = alloc_table(a.n_ent, ki, "cuda")
    rel = alloc_table(64, ki, "cuda")
    ent.copy_(torch.empty((a.n_ent, ki), device="cuda").normal_(0.0, a.sigma, generator=g))
    rel.copy_(torch.empty((64, ki), device="cuda").normal_(0.0, a.sigma, generator=g))
    if kind == "trained-like":
        Q, _ = D.eval_build_queries(mid, ent, rel, ki, scale, torch.from_numpy(T).cuda(), L.EVAL_O)
        b, o = 0.15, torch.from_numpy(T[:, 2].astype(np.int64)).cuda()
        eo = ent[o]
        qh = Q[:, :ki] / Q[:, :ki].norm(dim=1, keepdim=True)
        ent[o] = (1 - b * b) ** 0.5 * eo + b * eo.norm(dim=1, keepdim=True) * qh
    return ent, rel


def bench_rank(a):
    ki = 2 * a.k
    rs = np.random.RandomState(0)
    T = np.stack([rs.randint(0, a.n_ent, a.nq), rs.randint(0, 64, a.nq), rs.permutation(a.n_ent)[:a.nq]], 1).astype(np.int32)
    for kind in ("random", "trained-like"):
        cases, kept = {}, {}
        for name, mid, scale in RANK_MODELS:
            ent, rel = rank_tables(mid, scale, a, kind, T)
            cases[name] = (mid, scale, ent, rel, derived_tables(mid, ent, rel, ki))
        for prec in (2, 0):
            wall, kern, last, ranks = {}, {}, {}, {}
            for rep in range(a.reps + 1):   # (repetition 0 warms up: code objects, scratch buffers, the probe)
                for name, (mid, scale, ent, rel, tabs) in cases.items():
                    st = {}
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    r = rank_triples_device(mid, ent, rel, ki, scale, T, "o", "worst", precision=prec, stats=st,
                                            ent_f16=tabs if prec == 2 else None, query_chunk=a.nq)
                    dt = time.perf_counter() - t0
                    if rep:
                        wall.setdefault(name, []).append(dt * 1e3)
                        kern.setdefault(name, []).append(st.get("count_ms", float("nan")))
                    last[name], ranks[name] = st, r
            for name in cases:
                st = last[name]
                und = st.get("pairs", 0) / float(a.nq * a.n_ent)
                print("ranking %-12s %-8s precision %d: wall %8.1f .. %8.1f ms  kernels %8.1f .. %8.1f ms  %9.0f ranks/s  undecided %.4f %%  "
                      "fallback %d  mean rank %.1f" % (kind, name, prec, min(wall[name]), max(wall[name]), min(kern[name]), max(kern[name]),
                                                       a.nq / (min(wall[name]) * 1e-3), 100 * und, st.get("fallback", 0), ranks[name].mean()), flush=True)
                kept[(name, prec)] = ranks[name]
        for name in cases:
            assert (kept[(name, 2)] == kept[(name, 0)]).all(), "precision 2 and precision 0 disagree for %s on %s tables" % (name, kind)
        del cases
        torch.cuda.empty_cache()


def bench_train(a):
    ki, B, eta, n_rel = 2 * a.k, 16384, 20, 1000
    rs = np.random.RandomState(1)
    n = B * a.steps
    X = np.stack([rs.randint(0, a.n_ent, n), rs.randint(0, n_rel, n), rs.randint(0, a.n_ent, n)], 1).astype(np.int32)
    trainers = {}
    for name, mid, scale in (("SimplE", L.SIMPLE, 0.5), ("RotatE", L.ROTATE, 1.0), ("ComplEx", L.COMPLEX, 1.0)):
        g = torch.Generator(device="cuda").manual_seed(2)
        ent = alloc_table(a.n_ent, ki, "cuda")
        rel = alloc_table(n_rel, ki, "cuda")
        ent.copy_(torch.empty((a.n_ent, ki), device="cuda").uniform_(-0.5, 0.5, generator=g))
        if mid == L.ROTATE:
            rel[:, :ki // 2] = torch.empty((n_rel, ki // 2), device="cuda").uniform_(-np.pi, np.pi, generator=g)
        else:
            rel.copy_(torch.empty((n_rel, ki), device="cuda").uniform_(-0.5, 0.5, generator=g))
        tr = Trainer(mid, ki, scale, ent, rel, eta, loss="nll", optimizer="sgd", optimizer_params={"lr": 0.0005}, batches_count=a.steps, seed=0)
        tr.set_training_set(X, B)
        trainers[name] = tr
        print("  %-8s generic %s fused %s inplace %s factored %s" % (name, tr.generic, tr.fused, tr.inplace, tr.factored), flush=True)
    times = {}
    for rnd in range(a.reps + 1):   # (round 0 warms up: library load, allocations, the plan)
        for name, tr in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.run_batches([(b * B, B, rnd + 1, b + 1) for b in range(a.steps)])
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / a.steps
            if rnd:
                times.setdefault(name, []).append(dt * 1e3)
            tr.read_loss()
    for name, t in times.items():
        print("training C3 shape %-8s k_int = %d: %8.3f .. %8.3f ms/step  %7.1f M triples/s" % (name, ki, min(t), max(t), B * (1 + eta) / (min(t) * 1e-3) / 1e6),
              flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n-ent", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=8192)
    ap.add_argument("--k", type=int, default=200)
    ap.add_argument("--sigma", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--skip-rank", action="store_true")
    ap.add_argument("--skip-train", action="store_true")
    a = ap.parse_args()
    D.require_gpu()
    print("device %s  |E| = %d  k = %d" % (torch.cuda.get_device_name(0), a.n_ent, a.k), flush=True)
    if not a.skip_rank:
        bench_rank(a)
    if not a.skip_train:
        bench_train(a)


if __name__ == "__main__":
    main()
