#!/usr/bin/env python
"""Sampled ranking: the list-count kernel against the two routes that existed before it (DESIGN.md 4.2 "Ranking against given
candidates").

|E| = 1M, k = 200 (ComplEx and RotatE k_int = 400, TransE-L1 k_int = 200), 8192 test triples on both sides = 16384 query rows, K = 500
and 1000 drawn candidates per row.  Random tables only.  Per model and K, KERNEL time by HIP events around the one launch, one
warm-up of each, then --reps rounds that ALTERNATE the three routes on the same query rows and the same lists:

  (new)     emg_eval_count_lists;
  (filter)  emg_eval_filter_count fed the lists as its CSR (one lane per entry, rows read straight from memory);
  (rescore) emg_eval_rescore_pairs fed 8-byte pair records built from the lists, one segment per query row (the per-pair form).

The counters of the three are compared for equality on the spot (the run fails if they differ).  A fourth figure: the whole 1-vs-all
rank_triples_device call (precision 'auto') on the same triples, wall clock and its count_ms.

Verdict per (model, K): the kernel earns its place when the slowest of its runs is faster than the fastest run of the faster
existing route — the ranges of the alternating runs do not overlap; the margin is the spread those runs show.  Achieved bytes/s are
pairs x 4 k_int bytes (the gather floor: every candidate row read once) over the best kernel time, against ~6.3 TB/s of achievable
HBM bandwidth.  The run exits non-zero if a verdict is negative.

    python tools/bench_sampled_ranking.py [--n-ent 1000000] [--k 200] [--triples 8192] [--cands 500 1000] [--reps 4]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from emgraph_amd import _lib as L  # noqa: E402
from emgraph_amd import device as D  # noqa: E402
from emgraph_amd.evaluation.ranking import rank_triples_device  # noqa: E402
from emgraph_amd.training import alloc_table  # noqa: E402

HBM_ACHIEVABLE = 6.3e12   # bytes / s
CASES = {"ComplEx": (L.COMPLEX, 2), "TransE-L1": (L.TRANSE_L1, 1), "RotatE": (L.ROTATE, 2)}   # model id, k_int / k


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-ent", type=int, default=1000000)
    ap.add_argument("--n-rel", type=int, default=100)
    ap.add_argument("--k", type=int, default=200)
    ap.add_argument("--triples", type=int, default=8192)
    ap.add_argument("--cands", type=int, nargs="+", default=[500, 1000])
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--full-reps", type=int, default=2, help="timed repetitions of the 1-vs-all call (0: skip it)")
    ap.add_argument("--models", nargs="+", default=list(CASES))
    a = ap.parse_args()
    D.require_gpu()
    rs = np.random.RandomState(0)
    n_ent, n_rel, n = a.n_ent, a.n_rel, a.triples
    T = np.stack([rs.randint(0, n_ent, n), rs.randint(0, n_rel, n), rs.randint(0, n_ent, n)], 1).astype(np.int32)
    ok = True
    for name in a.models:
        mid, mult = CASES[name]
        ki = mult * a.k
        g = torch.Generator(device="cuda").manual_seed(1)
        ent, rel = alloc_table(n_ent, ki, "cuda"), alloc_table(n_rel, ki, "cuda")
        ent.copy_(torch.empty((n_ent, ki), device="cuda").uniform_(-0.5, 0.5, generator=g))
        rel.copy_(torch.empty((n_rel, ki), device="cuda").uniform_(-0.5, 0.5, generator=g))
        Q, pos_int = D.eval_build_queries(mid, ent, rel, ki, 1.0, torch.from_numpy(T).cuda(), L.EVAL_S_O)
        n_rows = Q.shape[0]
        full = {}
        if a.full_reps > 0:
            call = lambda st=None: rank_triples_device(mid, ent, rel, ki, 1.0, T, "s,o", "worst", precision="auto", stats=st)  # noqa: E731
            call()
            best = float("inf")
            for _ in range(a.full_reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                torch.cuda.synchronize()
                best = min(best, time.perf_counter() - t0)
            st = {}
            call(st)
            full = {"full_1vsall_call_ms": round(best * 1e3, 2), "full_1vsall_count_ms": round(st["count_ms"], 2)}
        for K in a.cands:
            cand = D.eval_draw_candidates(n, 0, L.EVAL_S_O, K, n_ent, 7, "cuda")
            ptr = torch.arange(n_rows + 1, dtype=torch.int64, device="cuda") * K
            idx = cand.reshape(-1).contiguous()
            pairs = ((torch.arange(n_rows, dtype=torch.int64, device="cuda") << 32)[:, None] | cand.long()).reshape(-1).contiguous()
            pcount = torch.full((n_rows + 1,), K, dtype=torch.int32, device="cuda")
            pcount[n_rows] = 0   # (the overflow flag of the prefilter that would have written the pairs)
            cnt = {r: torch.zeros((2, n_rows), dtype=torch.int32, device="cuda") for r in ("new", "filter", "rescore")}
            routes = {
                "new": lambda c: D.eval_count_lists(mid, Q, pos_int, ent, ki, 1.0, cand, c[0], c[1]),
                "filter": lambda c: D.eval_filter_count(mid, Q, pos_int, ent, 0, ki, 1.0, ptr, idx, c[0], c[1]),
                "rescore": lambda c: D.eval_rescore_pairs(mid, Q, pos_int, ent, 0, ki, 1.0, pairs, pcount, n_rows, c[0], c[1]),
            }
            for r, fn in routes.items():   # warm-up; its counters are the ones compared
                fn(cnt[r])
            torch.cuda.synchronize()
            if not (torch.equal(cnt["new"], cnt["filter"]) and torch.equal(cnt["new"], cnt["rescore"])):
                raise SystemExit("%s K=%d: the counters of the three routes differ" % (name, K))
            scratch = torch.zeros((2, n_rows), dtype=torch.int32, device="cuda")
            ms = {r: [] for r in routes}
            for _ in range(a.reps):
                for r, fn in routes.items():
                    ms[r].append(timed(lambda: fn(scratch)))
            old = min(("filter", "rescore"), key=lambda r: min(ms[r]))
            earns = max(ms["new"]) < min(ms[old])
            ok = ok and earns
            n_pairs, row_bytes = n_rows * K, 4 * ki
            rate = n_pairs * row_bytes / (min(ms["new"]) * 1e-3)
            res = {"model": name, "n_ent": n_ent, "k_int": ki, "rows": n_rows, "K": K, "pairs": n_pairs, "counters_equal": True,
                   "new_ms": [round(v, 3) for v in ms["new"]], "filter_count_ms": [round(v, 3) for v in ms["filter"]],
                   "rescore_pairs_ms": [round(v, 3) for v in ms["rescore"]], "faster_existing_route": old,
                   "ranges_disjoint_in_favour_of_new": bool(earns), "speedup_best_over_best": round(min(ms[old]) / min(ms["new"]), 2),
                   "gather_bytes": n_pairs * row_bytes, "new_bytes_per_s": round(rate), "share_of_achievable_hbm": round(rate / HBM_ACHIEVABLE, 3),
                   "new_pairs_per_s": round(n_pairs / (min(ms["new"]) * 1e-3))}
            res.update(full)
            print(json.dumps(res), flush=True)
        del ent, rel, Q
    if not ok:
        raise SystemExit("the list-count kernel did not beat the faster existing route outside the spread of the runs")


if __name__ == "__main__":
    main()
