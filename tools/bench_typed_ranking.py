#!/usr/bin/env python
"""Typed ranking throughput (DESIGN.md 4.2 "Typed ranking").

|E| = 1M, k = 200, ComplEx (k_int = 400) and TransE-L1 (k_int = 200), 1345 relations, 8192 test triples, 's,o'; per relation a
domain and a range pool of random entities, sizes log-uniform between 1k and 200k.  Random tables only.  Two things are timed, wall
clock around the whole call (host work, transfers and the device-to-host copy included), one warm-up, best of --reps:

  (a) the typed call: rank_triples_device(..., type_constraints=tc) — every pool of a query chunk in one launch;
  (b) the per-(relation, side) loop over entities_subset: what the typed call replaces (2 x #relations-met calls, each with its
      own query build and launch).  The loop uses nothing newer than entities_subset: --loop-only runs it alone on a checkout
      that has no type constraints (the baseline of the comparison; run both checkouts alternately on one box).

The two sets of ranks are compared on the spot (the run fails if they differ).  Reported per model: ranks/s of both, pairs/s of
the typed call against sum rows x |pool|, and the share of the f32 VALU issue rate that implies (39.3 T instr * lane / s, DESIGN.md
4.2) from the vector instructions of the tile's k loop per (pair, coordinate): 1 for the contraction (v_fma_f32), 2 for TransE-L1
(v_sub_f32, v_add_f32 with the |x| modifier).

    python tools/bench_typed_ranking.py [--n-ent 1000000] [--k 200] [--n-rel 1345] [--triples 8192] [--reps 4] [--loop-only]
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

VALU_RATE = 39.3e12   # instr * lane / s
CASES = {"ComplEx": (L.COMPLEX, 2, 1.0), "TransE-L1": (L.TRANSE_L1, 1, 2.0)}   # model id, k_int / k, instructions per (pair, coordinate)


def best_of(fn, reps):
    fn()   # warm-up
    best, out = float("inf"), None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-ent", type=int, default=1000000)
    ap.add_argument("--k", type=int, default=200)
    ap.add_argument("--n-rel", type=int, default=1345)
    ap.add_argument("--triples", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--pool-min", type=int, default=1000)
    ap.add_argument("--pool-max", type=int, default=200000)
    ap.add_argument("--models", nargs="+", default=list(CASES))
    ap.add_argument("--loop-only", action="store_true", help="time the entities_subset loop alone (a checkout without type constraints)")
    a = ap.parse_args()
    D.require_gpu()
    rs = np.random.RandomState(0)
    n_ent, n_rel = a.n_ent, a.n_rel
    hi = min(a.pool_max, n_ent)
    sizes = np.exp(rs.uniform(np.log(min(a.pool_min, hi)), np.log(hi), 2 * n_rel)).astype(np.int64)

    def pool(m):   # m distinct scattered ids: an arithmetic progression modulo n_ent with a random start and a stride coprime to n_ent
        stride = int(rs.randint(1, n_ent))
        while np.gcd(stride, n_ent) != 1:
            stride = int(rs.randint(1, n_ent))
        return np.sort((int(rs.randint(n_ent)) + stride * np.arange(m, dtype=np.int64)) % n_ent).astype(np.int32)

    pools = [pool(int(m)) for m in sizes]
    p = rs.randint(0, n_rel, a.triples)
    T = np.stack([np.array([pools[2 * q][rs.randint(len(pools[2 * q]))] for q in p]), p,
                  np.array([pools[2 * q + 1][rs.randint(len(pools[2 * q + 1]))] for q in p])], 1).astype(np.int32)
    pairs = int(sizes[2 * p].sum() + sizes[2 * p + 1].sum())
    tc = None
    if not a.loop_only:
        from emgraph_amd.evaluation import TypeConstraints
        ptr = np.zeros(2 * n_rel + 1, np.int64)
        np.cumsum(sizes, out=ptr[1:])
        tc = TypeConstraints(ptr, np.concatenate(pools), n_ent, n_rel)
    met = np.unique(p)
    rows_of = {int(q): np.flatnonzero(p == q) for q in met}
    for name in a.models:
        mid, mult, instr = CASES[name]
        ki = mult * a.k
        g = torch.Generator(device="cuda").manual_seed(1)
        ent, rel = alloc_table(n_ent, ki, "cuda"), alloc_table(n_rel, ki, "cuda")
        ent.copy_(torch.empty((n_ent, ki), device="cuda").uniform_(-0.5, 0.5, generator=g))
        rel.copy_(torch.empty((n_rel, ki), device="cuda").uniform_(-0.5, 0.5, generator=g))

        def loop():
            out = np.zeros((len(T), 2), np.int64)
            for q, rows in rows_of.items():
                for col, side in ((0, "s"), (1, "o")):
                    out[rows, col] = rank_triples_device(mid, ent, rel, ki, 1.0, T[rows], side, "worst",
                                                         entities_subset=pools[2 * q + col], precision=0)
            return out

        res = {"model": name, "n_ent": n_ent, "k_int": ki, "relations": n_rel, "relations_met": int(len(met)), "triples": len(T),
               "pairs": pairs, "loop_calls": 2 * int(len(met))}
        t_loop, want = best_of(loop, a.reps)
        res.update(loop_s=round(t_loop, 4), loop_ranks_per_s=round(2 * len(T) / t_loop))
        if tc is not None:
            stats = {}
            t_typed, got = best_of(lambda: rank_triples_device(mid, ent, rel, ki, 1.0, T, "s,o", "worst", type_constraints=tc), a.reps)
            rank_triples_device(mid, ent, rel, ki, 1.0, T, "s,o", "worst", type_constraints=tc, stats=stats)
            if not np.array_equal(got, want):
                raise SystemExit("%s: the typed ranks differ from the entities_subset loop's on %d rows" % (name, int((got != want).any(1).sum())))
            assert stats["typed_pairs"] == pairs
            res.update(typed_s=round(t_typed, 4), typed_ranks_per_s=round(2 * len(T) / t_typed), speedup=round(t_loop / t_typed, 2),
                       count_ms=round(stats["count_ms"], 3), pairs_per_s=round(pairs / (stats["count_ms"] * 1e-3)),
                       valu_share=round(pairs / (stats["count_ms"] * 1e-3) * ki * instr / VALU_RATE, 3), ranks_equal=True)
        print(json.dumps(res), flush=True)
        del ent, rel


if __name__ == "__main__":
    main()
