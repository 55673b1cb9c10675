#!/usr/bin/env python
"""Time the exact DBSCAN of find_clusters (emg_rows_dbscan) on 131 072 x 200 random-normal rows with planted blobs, against
the count-only l2 self-join (emg_rows_within, no pairs) on the same table — DBSCAN's count pass IS that join, and what the
link pass costs above it is its atomics and its border lists.

Device events around each repetition, one warm-up, the median of the repetitions, for the whole call and for the join alone.
The split of the call into count pass / link pass / finish comes from one further run under the torch profiler (device kernel
times summed by kernel name); without a usable profiler the split is reported as null and link + finish as the difference of
the two event timings.  Also reported: clusters, noise rows, core rows, and the longest parent chain the finish walked (the
first int64 of the workspace).  Prints one JSON line; needs a GPU."""
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
    """{count, link, finish} device ms of one call by kernel name, or None"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        split = {"count": 0.0, "link": 0.0, "finish": 0.0}
        for ev in prof.key_averages():
            us = float(getattr(ev, "device_time_total", 0.0) or getattr(ev, "cuda_time_total", 0.0) or 0.0)
            if "rows_within_kernel" in ev.key:
                split["count"] += us / 1e3
            elif "dbscan_link_kernel" in ev.key:
                split["link"] += us / 1e3
            elif "dbscan_" in ev.key:
                split["finish"] += us / 1e3     # init, roots, scan, rank, labels
        return split if split["count"] > 0 and split["link"] > 0 else None
    except Exception as exc:   # noqa: BLE001  (the profiler is optional: say why the split is missing)
        print("profiler unavailable: %r" % (exc,), file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=131072)
    ap.add_argument("--k", type=int, default=200)
    ap.add_argument("--blobs", type=int, default=64, help="planted blobs")
    ap.add_argument("--blob-rows", type=int, default=256, help="rows per blob")
    ap.add_argument("--blob-sigma", type=float, default=0.05, help="per-coordinate spread of a blob around its centre")
    ap.add_argument("--eps", type=float, default=2.0,
                    help="two rows of a blob are about sigma sqrt(2 k) = 1 apart, two random rows about sqrt(2 k) = 20")
    ap.add_argument("--min-samples", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    D.require_gpu()
    g = torch.Generator(device="cuda").manual_seed(1)
    X = torch.randn((args.n, args.k), generator=g, device="cuda", dtype=torch.float32)
    planted = min(args.blobs * args.blob_rows, args.n)
    if planted:   # blob b takes the rows b, b + blobs, b + 2 blobs, ... of a random selection: a cluster spans the whole table
        rows = torch.randperm(args.n, generator=g, device="cuda")[:planted]
        centres = torch.randn((args.blobs, args.k), generator=g, device="cuda", dtype=torch.float32)
        noise = torch.randn((planted, args.k), generator=g, device="cuda", dtype=torch.float32) * args.blob_sigma
        X[rows] = centres[torch.arange(planted, device="cuda") % args.blobs] + noise
    eps = float(np.float32(args.eps))
    ws = torch.empty(D.rows_dbscan_ws_bytes(args.n, args.min_samples), dtype=torch.uint8, device="cuda")

    def join():
        return D.rows_within(L.METRIC_L2, X, X, args.k, 0, eps)

    def dbscan():
        return D.rows_dbscan(X, args.k, L.METRIC_L2, eps, args.min_samples, ws=ws)

    j_ms, j_all, _ = timed(join, args.warmup, args.reps)
    d_ms, d_all, (labels, is_core, info) = timed(dbscan, args.warmup, args.reps)
    split = kernel_split(dbscan)
    clusters, noise_rows = info.cpu().tolist()
    out = {
        "n": args.n, "k_int": args.k, "eps": eps, "min_samples": args.min_samples,
        "planted_blobs": args.blobs, "planted_rows_per_blob": args.blob_rows,
        "join_count_only_ms_median": j_ms, "join_count_only_ms_all": j_all,
        "dbscan_ms_median": d_ms, "dbscan_ms_all": d_all,
        "link_plus_finish_ms_by_difference": d_ms - j_ms,
        "count_pass_ms": split and split["count"], "link_pass_ms": split and split["link"], "finish_ms": split and split["finish"],
        "link_pass_over_count_only_join": split and split["link"] / j_ms,
        "clusters": clusters, "noise_rows": noise_rows, "core_rows": int(is_core.sum()),
        "rows_labelled": int((labels >= 0).sum()),
        "longest_parent_chain": int(ws[:8].view(torch.int64).item()),
        "workspace_bytes": ws.numel(),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
