#!/usr/bin/env python
"""Time one Lloyd iteration of the device k-means (emg_rows_kmeans) at the C3 table shape — 1 M rows x 400 columns of random
normals, n_clusters 6, 64 and 1024 — and set it against the byte floor of its passes and, for n_clusters = 6, against the host
path it replaces (a host copy of the table plus sklearn.cluster.KMeans with the same start and n_init = 1).

A run of ``--iters`` updates from random rows as the start, tol = 0 (random data does not converge that fast: the run is checked
to have done all its updates).  Device events around each repetition, one warm-up, the median; per iteration = (the run - a
max_iter = 0 run) / iters.  The split into assign / update (counting sort, chunk sums, centres) / rest comes from one further
run under the torch profiler (device kernel times summed by kernel name); `rocprofv3 --kernel-trace --stats -- python
tools/bench_kmeans.py --no-profiler` gives the same split from outside.  Byte floor: the two passes of an iteration that read
the table (assign, chunk sums), n * width * 4 bytes each, at the 6.0 TB/s an in-order sweep of HBM reaches on this card
(DESIGN.md 7).  Prints one JSON line per n_clusters; needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from emgraph_amd import device as D  # noqa: E402

SWEEP_TBS = 6.0


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


def kernel_split(fn, iters):
    """device ms per iteration by kernel family, or None"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        split = {"assign": 0.0, "sort": 0.0, "chunk_sums": 0.0, "centres": 0.0, "rest": 0.0}
        for ev in prof.key_averages():
            us = float(getattr(ev, "device_time_total", 0.0) or getattr(ev, "cuda_time_total", 0.0) or 0.0)
            key = ev.key
            if "kmeans_assign_kernel" in key:
                split["assign"] += us / 1e3
            elif any(name in key for name in ("kmeans_hist", "kmeans_colscan", "kmeans_starts", "kmeans_scatter")):
                split["sort"] += us / 1e3
            elif "kmeans_chunk_kernel<0>" in key or "kmeans_chunk_kernelILi0" in key:
                split["chunk_sums"] += us / 1e3
            elif "kmeans_centres" in key:
                split["centres"] += us / 1e3
            elif "kmeans_" in key:
                split["rest"] += us / 1e3        # state, tolerance passes, decide, inertia, info: per run, not per iteration
        if split["assign"] <= 0:
            return None
        split["assign"] *= iters / (iters + 1.0)   # a run makes iters + 1 assignments
        return {name: ms / iters for name, ms in split.items()}
    except Exception as exc:   # noqa: BLE001  (the profiler is optional: say why the split is missing)
        print("profiler unavailable: %r" % (exc,), file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--width", type=int, default=400)
    ap.add_argument("--clusters", type=int, nargs="+", default=[6, 64, 1024])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sklearn", action="store_true", help="also time the host path for the first n_clusters")
    ap.add_argument("--no-profiler", action="store_true")
    args = ap.parse_args()
    D.require_gpu()
    g = torch.Generator(device="cuda").manual_seed(1)
    X = torch.randn((args.n, args.width), generator=g, device="cuda", dtype=torch.float32)
    pass_bytes = args.n * args.width * 4
    for C in args.clusters:
        start = X[torch.randperm(args.n, generator=g, device="cuda")[:C]].contiguous()
        ws = torch.empty(D.rows_kmeans_ws_bytes(args.n, C, args.width), dtype=torch.uint8, device="cuda")

        def run(max_iter=args.iters):
            return D.rows_kmeans(X, args.width, start.clone(), max_iter, 0.0, ws=ws)

        r_ms, r_all, (_, info) = timed(run, args.warmup, args.reps)
        a_ms, a_all, _ = timed(lambda: run(0), args.warmup, args.reps)
        inertia, n_iter, converged, _ = D.kmeans_info(info)
        split = None if args.no_profiler else kernel_split(run, args.iters)
        out = {
            "n": args.n, "width": args.width, "n_clusters": C, "iters": args.iters, "updates_done": n_iter, "converged": converged,
            "run_ms_median": r_ms, "run_ms_all": r_all, "assign_only_run_ms_median": a_ms,
            "ms_per_iteration": (r_ms - a_ms) / args.iters,
            "split_ms_per_iteration": split,
            "table_pass_bytes": pass_bytes, "byte_floor_ms_per_iteration": 2 * pass_bytes / (SWEEP_TBS * 1e12) * 1e3,
            "assign_pass_floor_ms": pass_bytes / (SWEEP_TBS * 1e12) * 1e3,
            "workspace_bytes": ws.numel(), "inertia": inertia,
        }
        if args.sklearn and C == args.clusters[0]:
            from sklearn.cluster import KMeans
            t0 = time.perf_counter()
            host = X.cpu().numpy()
            t1 = time.perf_counter()
            fit = KMeans(C, init=start.cpu().numpy(), n_init=1, max_iter=args.iters, tol=0, algorithm="lloyd").fit(host)
            t2 = time.perf_counter()
            out.update({"host_copy_ms": (t1 - t0) * 1e3, "sklearn_fit_ms": (t2 - t1) * 1e3, "sklearn_n_iter": int(fit.n_iter_),
                        "sklearn_ms_per_iteration": (t2 - t1) * 1e3 / max(int(fit.n_iter_), 1),
                        "sklearn_threads": os.environ.get("OMP_NUM_THREADS"), "sklearn_inertia": float(fit.inertia_)})
        print(json.dumps(out), flush=True)
        del ws


if __name__ == "__main__":
    main()
