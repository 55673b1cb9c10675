#!/usr/bin/env python
"""RotatE next to its nearest yardsticks, same device, same run.

Exact ranking: 8192 test triples x 1M entities, k = 200 (k_int = 400), object side, rank_triples_device at precision 0 — RotatE's
tiled exact kernel (count_rotate_kernel) next to TransE-L1's exact kernel at k_int = 400; alternating, best of --reps.
Training: the C3 shape (B = 16384, eta = 20, |E| = 1M, |R| = 1000, k_int = 400, nll, SGD), ms per step of the Trainer — RotatE
next to TransE(norm = 3), the other model of the generic step; alternating rounds, best round.

    python tools/bench_rotate.py [--n-ent 1000000] [--nq 8192] [--k 200] [--reps 4] [--steps 20] [--skip-train] [--skip-rank]
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
from emgraph_amd.evaluation.ranking import rank_triples_device  # noqa: E402
from emgraph_amd.training import Trainer, alloc_table  # noqa: E402


def tables(model, n_ent, n_rel, ki, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    ent = alloc_table(n_ent, ki, "cuda")
    rel = alloc_table(n_rel, ki, "cuda")
    ent.copy_(torch.empty((n_ent, ki), device="cuda").uniform_(-0.5, 0.5, generator=g))
    if model == L.ROTATE:
        rel[:, :ki // 2] = torch.empty((n_rel, ki // 2), device="cuda").uniform_(-np.pi, np.pi, generator=g)
    else:
        rel.copy_(torch.empty((n_rel, ki), device="cuda").uniform_(-0.5, 0.5, generator=g))
    return ent, rel


def bench_rank(a):
    ki = 2 * a.k
    rs = np.random.RandomState(0)
    T = np.stack([rs.randint(0, a.n_ent, a.nq), rs.randint(0, 64, a.nq), rs.randint(0, a.n_ent, a.nq)], 1).astype(np.int32)
    cases = {"RotatE": (L.ROTATE,) + tables(L.ROTATE, a.n_ent, 64, ki, 0), "TransE-L1": (L.TRANSE_L1,) + tables(L.TRANSE_L1, a.n_ent, 64, ki, 0)}
    best = {}
    for rep in range(a.reps):
        for name, (mid, ent, rel) in cases.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = rank_triples_device(mid, ent, rel, ki, 1.0, T, "o", "worst", precision=0, query_chunk=a.nq)
            dt = time.perf_counter() - t0
            best[name] = min(best.get(name, dt), dt)
            print("  rep %d %-10s %9.1f ms  mean rank %.1f" % (rep, name, dt * 1e3, r.mean()), flush=True)
    for name, dt in best.items():
        print("exact ranking %-10s k_int = %d: %9.1f ms  %10.0f ranks/s" % (name, ki, dt * 1e3, a.nq / dt), flush=True)


def bench_train(a):
    ki, B, eta, n_rel = 2 * a.k, 16384, 20, 1000
    rs = np.random.RandomState(1)
    n = B * a.steps
    X = np.stack([rs.randint(0, a.n_ent, n), rs.randint(0, n_rel, n), rs.randint(0, a.n_ent, n)], 1).astype(np.int32)
    trainers = {}
    for name, mid, scale in (("RotatE", L.ROTATE, 1.0), ("TransE(norm=3)", L.TRANSE_P, 3.0)):
        ent, rel = tables(mid, a.n_ent, n_rel, ki, 2)
        tr = Trainer(mid, ki, scale, ent, rel, eta, loss="nll", optimizer="sgd", optimizer_params={"lr": 0.0005}, batches_count=a.steps, seed=0)
        tr.set_training_set(X, B)
        trainers[name] = tr
    best = {}
    for rnd in range(a.reps + 1):   # (round 0 warms up: library load, allocations, the plan)
        for name, tr in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.run_batches([(b * B, B, rnd + 1, b + 1) for b in range(a.steps)])
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / a.steps
            if rnd:
                best[name] = min(best.get(name, dt), dt)
            print("  round %d %-15s %8.3f ms/step" % (rnd, name, dt * 1e3), flush=True)
            tr.read_loss()
    for name, dt in best.items():
        print("training C3 shape %-15s k_int = %d: %8.3f ms/step  %7.1f M triples/s" % (name, ki, dt * 1e3, B * (1 + eta) / dt / 1e6), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n-ent", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=8192)
    ap.add_argument("--k", type=int, default=200)
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
