#!/usr/bin/env python
"""Time the l2 self-join of discovery (emg_rows_within: count + nearest other row, no pairs) against the same join done with
torch.cdist(compute_mode="donot_use_mm_for_euclid_dist") in row chunks plus a threshold.

Device events around each repetition, one warm-up, the median of the repetitions.  The torch form is timed on the first
``--torch-rows`` query rows against the whole table and scaled to all rows (its cost is linear in the query rows; the
scaling is reported, not hidden).  Prints one JSON line; needs a GPU."""
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

PEAK_F32_VALU = 157.3e12   # FLOP/s, MI355X vector f32 (data sheet)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=131072)
    ap.add_argument("--k", type=int, default=200)
    ap.add_argument("--radius", type=float, default=18.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--torch-rows", type=int, default=8192)
    ap.add_argument("--torch-chunk", type=int, default=64,
                    help="query rows per cdist call: that form launches one workgroup of 256 threads per distance, and a "
                         "launch holds fewer than 2^32 threads (64 rows x 131072 = 2^31)")
    args = ap.parse_args()
    D.require_gpu()
    g = torch.Generator(device="cuda").manual_seed(1)
    X = torch.randn((args.n, args.k), generator=g, device="cuda", dtype=torch.float32)
    radius = float(np.float32(args.radius))

    def kernel():
        return D.rows_within(L.METRIC_L2, X, X, args.k, 0, radius)

    k_ms, k_all, (count, nn_dist, nn_id, _, _) = timed(kernel, args.warmup, args.reps)

    print(json.dumps({"kernel_ms_median": k_ms, "kernel_ms_all": k_all}), file=sys.stderr, flush=True)
    rows = min(args.torch_rows, args.n)
    if (args.torch_chunk * args.n) * 256 >= 2 ** 32:
        raise SystemExit("--torch-chunk %d x n %d x 256 threads does not fit one launch" % (args.torch_chunk, args.n))

    def chunked():
        cnt, nnd, nni = [], [], []
        for c0 in range(0, rows, args.torch_chunk):
            c1 = min(c0 + args.torch_chunk, rows)
            d = torch.cdist(X[c0:c1], X, compute_mode="donot_use_mm_for_euclid_dist")
            ar = torch.arange(c1 - c0, device="cuda")
            d[ar, c0 + ar] = float("inf")
            cnt.append((d <= radius).sum(1))
            m = d.min(1)
            nnd.append(m.values)
            nni.append(m.indices)
        return torch.cat(cnt), torch.cat(nnd), torch.cat(nni)

    t_ms, t_all, (t_cnt, t_nnd, t_nni) = timed(chunked, args.warmup, args.reps)
    flop = 3.0 * args.n * args.n * args.k
    out = {
        "n": args.n, "k_int": args.k, "radius": radius,
        "kernel_ms_median": k_ms, "kernel_ms_all": k_all,
        "kernel_tflops": flop / (k_ms * 1e-3) / 1e12,
        "kernel_fraction_of_f32_valu_peak": flop / (k_ms * 1e-3) / PEAK_F32_VALU,
        "torch_rows_timed": rows, "torch_ms_median_timed_rows": t_ms, "torch_ms_all": t_all,
        "torch_ms_scaled_to_all_rows": t_ms * args.n / rows,
        "kernel_speedup_over_torch": (t_ms * args.n / rows) / k_ms,
        # agreement on the timed rows (torch's per-pair sums are ordered differently: distances differ in the last bits)
        "count_equal_fraction": float((t_cnt.to(torch.int32) == count[:rows]).float().mean()),
        "nn_id_equal_fraction": float((t_nni.to(torch.int32) == nn_id[:rows]).float().mean()),
        "nn_dist_max_abs_diff": float((t_nnd - nn_dist[:rows]).abs().max()),
        "rows_with_a_neighbour_within_radius": int((count > 0).sum()),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
