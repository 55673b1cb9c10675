#!/usr/bin/env python
"""Relation prediction throughput (DESIGN.md 4.2 "Relation prediction").

1M (s, o) pairs against 1345 and against 237 candidate relations, |E| = 1M: ComplEx k = 200 (k_int = 400), TransE-L1 k = 200
(k_int = 200) and RotatE k = 200 (k_int = 400).  Timed with HIP events around the emg_eval_rel_count launches of the whole pair
list (chunks of 65536 rows, triples and pos_int already on the device), one chunk as warm-up, best of --reps; and once end to end
through rank_relations_device (host CSR, pos_int, the device-to-host copy included).  Every result comes with its fraction of
the VALU issue rate DESIGN.md uses (39.3 T instr * lane / s), from the vector instructions the compiled inner loop spends per
(pair, relation, coordinate) — the counts below are read off the gfx950 disassembly of rel_score_kernel's k loop (packed
f32 instructions count once).

    python tools/bench_relation_ranking.py [--pairs 1000000] [--n-ent 1000000] [--k 200] [--reps 4] [--rels 1345 237]
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
from emgraph_amd.evaluation.ranking import rank_relations_device  # noqa: E402
from emgraph_amd.training import alloc_table  # noqa: E402

VALU_RATE = 39.3e12   # instr * lane / s
CHUNK = 1 << 16
# name -> (model id, k_int / k, vector instructions of the wide form's k loop per (pair, relation) and coordinate of k_int)
#   ComplEx: 48 packed (32 fma + 16 mul) + 7 (pass 0) or 15 (pass 1) per 32 (relation, complex coordinate) steps of a pass, two passes
#   TransE-L1: 48 packed adds + 32 v_and (|x|: a packed instruction has no abs modifier) + 14 per 32 steps
#   RotatE: 727 per 32 (relation, complex coordinate) steps: 8 for q, the rest the unfused modulus with its correctly rounded sqrtf
CASES = {"ComplEx": (L.COMPLEX, 2, 59 / 32.0), "TransE-L1": (L.TRANSE_L1, 1, 94 / 32.0), "RotatE": (L.ROTATE, 2, 727 / 64.0)}

def tables(mid, n_ent, n_rel, ki, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    ent = alloc_table(n_ent, ki, "cuda")
    rel = alloc_table(n_rel, ki, "cuda")
    ent.copy_(torch.empty((n_ent, ki), device="cuda").uniform_(-0.5, 0.5, generator=g))
    if mid == L.ROTATE:
        rel[:, :ki // 2] = torch.empty((n_rel, ki // 2), device="cuda").uniform_(-np.pi, np.pi, generator=g)
    else:
        rel.copy_(torch.empty((n_rel, ki), device="cuda").uniform_(-0.5, 0.5, generator=g))
    return ent, rel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--n-ent", type=int, default=1000000)
    ap.add_argument("--k", type=int, default=200)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--rels", type=int, nargs="+", default=[1345, 237])
    ap.add_argument("--models", nargs="+", default=list(CASES))
    a = ap.parse_args()
    D.require_gpu()
    rs = np.random.RandomState(0)
    for name in a.models:
        mid, mult, instr = CASES[name]
        ki = mult * a.k
        for n_rel in a.rels:
            ent, rel = tables(mid, a.n_ent, n_rel, ki, 0)
            T = np.stack([rs.randint(0, a.n_ent, a.pairs), rs.randint(0, n_rel, a.pairs), rs.randint(0, a.n_ent, a.pairs)], 1).astype(np.int32)
            op = D.eval_rel_rotate_image(rel, ki) if mid == L.ROTATE else rel
            chunks = []
            for c0 in range(0, a.pairs, CHUNK):
                Tt = torch.from_numpy(T[c0:c0 + CHUNK]).cuda()
                _, pos = D.eval_build_queries(mid, ent, rel, ki, 1.0, Tt, L.EVAL_O)
                chunks.append((Tt, pos, torch.empty((4, Tt.shape[0]), dtype=torch.int32, device="cuda")))
            best = None
            D.eval_rel_count(mid, ent, op, ki, 1.0, chunks[0][0], chunks[0][1], cnt=chunks[0][2])   # warm-up: one chunk
            for rep in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for Tt, pos, cnt in chunks:
                    D.eval_rel_count(mid, ent, op, ki, 1.0, Tt, pos, cnt=cnt)
                e1.record()
                torch.cuda.synchronize()
                ms = e0.elapsed_time(e1)
                best = ms if best is None else min(best, ms)
            del chunks
            scores = a.pairs * n_rel / (best * 1e-3)
            frac = scores * ki * instr / VALU_RATE
            t0 = time.perf_counter()
            r = rank_relations_device(mid, ent, rel, ki, 1.0, T, "worst")
            e2e = time.perf_counter() - t0
            print("%-10s k_int %3d  %7d pairs x %4d relations: kernel %8.1f ms  %9.0f ranks/s  %6.2f G scores/s  %4.1f %% of the VALU issue rate"
                  "  | end to end %8.1f ms %9.0f ranks/s  mean rank %.1f"
                  % (name, ki, a.pairs, n_rel, best, a.pairs / (best * 1e-3), scores / 1e9, 100 * frac, e2e * 1e3, a.pairs / e2e, r.mean()),
                  flush=True)
            del ent, rel, op
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
