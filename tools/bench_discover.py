#!/usr/bin/env python
"""Time the grid ranking of discover_facts (ranking.grid_ranks_device -> emg_eval_grid_count) on one relation of a ComplEx model
with 131 072 entities, k = 200, and a 110 x 110 grid, against rank_triples_device on the same 12 100 cells — the way to the same
ranks without the grid kernel: 24 200 rows of 1-vs-all scoring where the grid scores 220.

Device events around each repetition, one warm-up, the median of the repetitions; both calls include their host work (filter
CSR, copies).  rank_triples_device runs at precision 'auto' (what evaluate_performance picks) and at precision 0 (the exact f32
kernel alone).  The split of the grid call by kernel comes from one further run under the torch profiler (device kernel times
summed by kernel name), null without a usable profiler.  The two ways must give the same ranks on every cell that is not in
the filter: reported as ranks_equal.  Prints one JSON line; needs a GPU."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from emgraph_amd import _lib as L  # noqa: E402
from emgraph_amd import device as D  # noqa: E402
from emgraph_amd.evaluation.ranking import FilterIndex, grid_ranks_device, rank_triples_device  # noqa: E402


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), ms, out


def kernel_split(fn):
    """{thresholds, count, queries, other} device ms of one call by kernel name, or None"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        split = {"thresholds": 0.0, "count": 0.0, "queries": 0.0, "other": 0.0}
        for ev in prof.key_averages():
            us = float(getattr(ev, "device_time_total", 0.0) or getattr(ev, "cuda_time_total", 0.0) or 0.0)
            if "grid_thr_kernel" in ev.key:
                split["thresholds"] += us / 1e3
            elif "grid_mfma_kernel" in ev.key or "grid_transe_kernel" in ev.key:
                split["count"] += us / 1e3
            elif "build_queries" in ev.key:
                split["queries"] += us / 1e3
            else:
                split["other"] += us / 1e3     # copies, the sum gt + eq, concatenations
        return split if split["count"] > 0 else None
    except Exception as exc:   # noqa: BLE001  (the profiler is optional: say why the split is missing)
        print("profiler unavailable: %r" % (exc,), file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-ent", type=int, default=131072)
    ap.add_argument("--k", type=int, default=200)
    ap.add_argument("--grid", type=int, default=110, help="subjects and objects of the grid")
    ap.add_argument("--filter-triples", type=int, default=1_000_000, help="random known triples of the relation")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    D.require_gpu()
    ki = 2 * args.k
    g = torch.Generator(device="cuda").manual_seed(1)
    ent = torch.randn((args.n_ent, ki), generator=g, device="cuda", dtype=torch.float32) * 0.3
    rel = torch.randn((1, ki), generator=g, device="cuda", dtype=torch.float32) * 0.3
    rs = np.random.RandomState(2)
    S = np.sort(rs.choice(args.n_ent, args.grid, replace=False)).astype(np.int64)
    O = np.sort(rs.choice(args.n_ent, args.grid, replace=False)).astype(np.int64)
    X = np.stack([rs.randint(0, args.n_ent, args.filter_triples), np.zeros(args.filter_triples, np.int64),
                  rs.randint(0, args.n_ent, args.filter_triples)], 1)
    X[:args.grid, 0], X[:args.grid, 2] = S, O[::-1]   # some cells of the grid are known
    findex = FilterIndex(X)
    findex.known_csr(np.zeros((1, 2), np.int64), "o", args.n_ent)   # both sorted sides are built before anything is timed
    findex.known_csr(np.zeros((1, 2), np.int64), "s", args.n_ent)
    cells = np.stack([np.repeat(S, len(O)), np.zeros(len(S) * len(O), np.int64), np.tile(O, len(S))], 1)

    def grid():
        return grid_ranks_device(L.COMPLEX, ent, rel, ki, 1.0, 0, S, O, findex)

    def per_cell(precision):
        return lambda: rank_triples_device(L.COMPLEX, ent, rel, ki, 1.0, cells, "s,o", "worst", filter_triples=findex,
                                           precision=precision)

    g_ms, g_all, (rank_s, rank_o) = timed(grid, args.warmup, args.reps)
    a_ms, a_all, ranks = timed(per_cell("auto"), args.warmup, args.reps)
    e_ms, e_all, ranks0 = timed(per_cell(0), args.warmup, args.reps)
    split = kernel_split(grid)
    known = np.isin(cells[:, 0] * args.n_ent + cells[:, 2], X[:, 0] * args.n_ent + X[:, 2])
    got = np.stack([rank_s.reshape(-1), rank_o.reshape(-1)], 1)
    out = {
        "n_ent": args.n_ent, "k": args.k, "k_int": ki, "grid": [len(S), len(O)], "cells": len(cells),
        "known_cells": int(known.sum()), "filter_triples": len(X),
        "rows_scored_grid": len(S) + len(O), "rows_scored_per_cell": 2 * len(cells),
        "grid_ranks_ms_median": g_ms, "grid_ranks_ms_all": g_all,
        "rank_triples_auto_ms_median": a_ms, "rank_triples_auto_ms_all": a_all,
        "rank_triples_exact_f32_ms_median": e_ms, "rank_triples_exact_f32_ms_all": e_all,
        "grid_thresholds_kernel_ms": split and split["thresholds"], "grid_count_kernel_ms": split and split["count"],
        "grid_build_queries_ms": split and split["queries"], "grid_other_device_ms": split and split["other"],
        "ranks_equal": bool(np.array_equal(got[~known], ranks[~known]) and np.array_equal(ranks, ranks0)),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
