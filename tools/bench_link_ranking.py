#!/usr/bin/env python
"""Ranks per second of ranking THROUGH a score link at the C4 shape (DESIGN.md 4.2 "Ranking through a link").

8192 test triples x 1M entities, ComplEx k = 200, object side, on trained-like tables (N(0, sigma) with every test triple's
object aligned with its query vector: tools/eval_throughput.py's "planted" tables).  rank_triples_device under tanh at
precision 2 (half-precision prefilter with bisected thresholds) and precision 0 (exact kernel, the link in its epilogue), against
the linear figures of the same box and tables.  The ranks of the two precisions are compared (they must be equal).

    python tools/bench_link_ranking.py [--n-ent 1000000] [--nq 8192] [--k 200] [--sigma 0.1] [--link tanh] [--reps 4]
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n-ent", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=8192)
    ap.add_argument("--k", type=int, default=200)
    ap.add_argument("--sigma", type=float, default=0.1)
    ap.add_argument("--link", default="tanh", choices=["tanh", "sigmoid", "softplus"])
    ap.add_argument("--reps", type=int, default=4)
    a = ap.parse_args()
    D.require_gpu()
    ki = 2 * a.k
    g = torch.Generator(device="cuda").manual_seed(0)
    ent = torch.empty((a.n_ent, ki), device="cuda").normal_(0.0, a.sigma, generator=g)
    rel = torch.empty((64, ki), device="cuda").normal_(0.0, a.sigma, generator=g)
    rs = np.random.RandomState(0)
    T = np.stack([rs.randint(0, a.n_ent, a.nq), rs.randint(0, 64, a.nq), rs.permutation(a.n_ent)[:a.nq]], 1).astype(np.int32)
    Q, _ = D.eval_build_queries(L.COMPLEX, ent, rel, ki, 1.0, torch.from_numpy(T).cuda(), L.EVAL_O)
    b, o = 0.15, torch.from_numpy(T[:, 2].astype(np.int64)).cuda()
    eo = ent[o]
    qh = Q[:, :ki] / Q[:, :ki].norm(dim=1, keepdim=True)
    ent[o] = (1 - b * b) ** 0.5 * eo + b * eo.norm(dim=1, keepdim=True) * qh
    tabs = derived_tables(L.COMPLEX, ent, rel, ki)
    print("device %s  |E| = %d  nq = %d  ComplEx k = %d  sigma = %g" % (torch.cuda.get_device_name(0), a.n_ent, a.nq, a.k, a.sigma))
    ranks = {}
    for name, link in (("linear", L.LINK_LINEAR), (a.link, L.LINK_IDS[a.link])):
        for prec in (2, 0):
            best, st = None, {}
            for rep in range(a.reps):
                st = {}
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = rank_triples_device(L.COMPLEX, ent, rel, ki, 1.0, T, "o", "worst", precision=prec, link=link, stats=st,
                                        ent_f16=tabs if prec == 2 else None, query_chunk=a.nq)
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
            ranks[(name, prec)] = r
            print("%-8s precision %d: %8.1f ms  %10.0f ranks/s  mean rank %.1f  stats %s"
                  % (name, prec, best * 1e3, a.nq / best, r.mean(), {k: v for k, v in st.items() if k != "count_ms"}), flush=True)
        assert (ranks[(name, 2)] == ranks[(name, 0)]).all(), "precision 2 and precision 0 disagree under %s" % name


if __name__ == "__main__":
    main()
