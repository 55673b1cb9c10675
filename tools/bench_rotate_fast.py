#!/usr/bin/env python
"""RotatE exact-fast ranking next to the exact kernel (DESIGN.md 4.5 "Exact-fast ranking").

8192 test triples x 1M entities, k = 200 (k_int = 400), object side, two kinds of table:
  random   entity rows uniform in +-0.5, random positives (tools/bench_rotate.py's tables): the pessimistic case
  trained  N(0, sigma) rows with every test triple's object pulled towards its query row (tools/bench_link_ranking.py's "planted"
           tables, for a distance model: o <- q + b (o - q)): the positives rank near the top, as after a fit
Reported per table: the exact kernel (rank_triples_device, precision 0), the fast mode end to end (precision 'auto', the derived
tables kept as a fitted model keeps them), and of the fast mode the prefilter and the re-scoring alone (HIP events around each
launch), the undecided share and the prefilter's share of the VALU issue rate (4.5 issued instructions per (pair, coordinate), the
root counted twice: 5.5 issue slots of 64 lanes, against 4 SIMDs x 16 lanes per CU and cycle at --clock-mhz, the peak engine clock).  Best
of --reps, alternating.  --exact-only: the exact kernel alone — this file runs unchanged in a checkout without the fast mode, which is how
the baseline of a comparison across commits is taken (same box, same session).

    python tools/bench_rotate_fast.py [--n-ent 1000000] [--nq 8192] [--k 200] [--reps 4] [--tables random,trained] [--exact-only] [--clock-mhz 2400]
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

ISSUE_SLOTS = 5.5   # per (pair, coordinate): v_pk_add_f16, 2 v_fma_mix_f32, v_sqrt_f32 (two slots), half a v_pk_add_f32


def make_tables(kind, n_ent, ki, nq, sigma, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rel = torch.zeros((64, ki), device="cuda")
    rel[:, :ki // 2] = torch.empty((64, ki // 2), device="cuda").uniform_(-np.pi, np.pi, generator=g)
    rs = np.random.RandomState(seed)
    if kind == "random":
        ent = torch.empty((n_ent, ki), device="cuda").uniform_(-0.5, 0.5, generator=g)
        T = np.stack([rs.randint(0, n_ent, nq), rs.randint(0, 64, nq), rs.randint(0, n_ent, nq)], 1).astype(np.int32)
        return ent, rel, T
    ent = torch.empty((n_ent, ki), device="cuda").normal_(0.0, sigma, generator=g)
    perm = rs.permutation(n_ent)
    T = np.stack([perm[nq:2 * nq] if n_ent >= 2 * nq else rs.randint(0, n_ent, nq), rs.randint(0, 64, nq), perm[:nq]], 1).astype(np.int32)
    Q, _ = D.eval_build_queries(L.ROTATE, ent, rel, ki, 1.0, torch.from_numpy(T).cuda(), L.EVAL_O)
    o = torch.from_numpy(T[:, 2].astype(np.int64)).cuda()
    ent[o] = Q[:, :ki] + 0.55 * (ent[o] - Q[:, :ki])     # (subjects and objects are disjoint rows: the query rows do not move)
    return ent, rel, T


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def stages(ent, rel, T, ki, tabs):
    """(prefilter ms, re-scoring ms, undecided share) of one pass of the fast mode's two kernels, HIP events around each launch"""
    from emgraph_amd.evaluation.ranking import _pair_buffer
    Tt = torch.from_numpy(T).cuda()
    Q, pos_int = D.eval_build_queries(L.ROTATE, ent, rel, ki, 1.0, Tt, L.EVAL_O)
    Qh, rho_q, q_stats = D.eval_rotate_image(Q, ki, tabs.scale)
    thr = D.eval_rotate_thresholds(pos_int, rho_q, ki, tabs.scale, q_stats, tabs.ent_stats)
    n_rows, n_cand = Q.shape[0], ent.shape[0]
    n_seg = D.eval_prefilter_rotate_segments(n_rows, n_cand)
    pairs, pcount = _pair_buffer(ent.device, n_seg, cap_factor=4)
    cnt = torch.zeros((2, n_rows), dtype=torch.int32, device="cuda")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    ev[0].record()
    D.eval_prefilter_rotate(Qh, thr, tabs.ent_f16, 0, ki, cnt[0], pairs, pcount)
    ev[1].record()
    D.eval_rescore_pairs(L.ROTATE, Q, pos_int, ent, 0, ki, 1.0, pairs, pcount, n_seg, cnt[0], cnt[1], 4)
    ev[2].record()
    torch.cuda.synchronize()
    over, n_pairs = int(pcount[n_seg]), int(pcount[:n_seg].sum())
    return ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]), n_pairs / float(n_rows * n_cand), over


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n-ent", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=8192)
    ap.add_argument("--k", type=int, default=200)
    ap.add_argument("--sigma", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--tables", default="random,trained")
    ap.add_argument("--exact-only", action="store_true")
    ap.add_argument("--clock-mhz", type=float, default=2400.0)
    a = ap.parse_args()
    D.require_gpu()
    ki = 2 * a.k
    props = torch.cuda.get_device_properties(0)
    print("device %s  |E| = %d  nq = %d  RotatE k = %d  library %s" % (props.name, a.n_ent, a.nq, a.k, L.load().emg_source_hash().decode()), flush=True)
    for kind in a.tables.split(","):
        ent, rel, T = make_tables(kind, a.n_ent, ki, a.nq, a.sigma)
        run = lambda prec, st=None, tabs=None: rank_triples_device(L.ROTATE, ent, rel, ki, 1.0, T, "o", "worst", precision=prec,  # noqa: E731
                                                                   query_chunk=a.nq, stats=st, ent_f16=tabs)
        tabs = None
        if not a.exact_only:
            from emgraph_amd.evaluation.ranking import derived_tables
            t_tabs, tabs = timed(lambda: derived_tables(L.ROTATE, ent, rel, ki))
            print("%-8s derived tables (once per fitted model): %.1f ms  scale 2^%d  ok %s" % (kind, t_tabs * 1e3, int(np.log2(tabs.scale)), tabs.ok), flush=True)
        best, ranks, st, stage = {}, {}, {}, None
        for rep in range(a.reps):
            dt, ranks["exact"] = timed(lambda: run(0))
            best["exact"] = min(best.get("exact", dt), dt)
            print("  rep %d %-8s exact %9.1f ms" % (rep, kind, dt * 1e3), flush=True)
            if a.exact_only:
                continue
            st = {}
            dt, ranks["fast"] = timed(lambda: run("auto", st, tabs))
            best["fast"] = min(best.get("fast", dt), dt)
            s = stages(ent, rel, T, ki, tabs)
            stage = s if stage is None else (min(stage[0], s[0]), min(stage[1], s[1]), s[2], s[3])
            print("  rep %d %-8s fast  %9.1f ms   prefilter %.1f ms  re-scoring %.1f ms" % (rep, kind, dt * 1e3, s[0], s[1]), flush=True)
        print("%-8s exact kernel : %9.1f ms  %10.0f ranks/s  mean rank %.1f" % (kind, best["exact"] * 1e3, a.nq / best["exact"], ranks["exact"].mean()), flush=True)
        if a.exact_only:
            continue
        assert (ranks["fast"] == ranks["exact"]).all(), "the fast mode and the exact kernel disagree"
        slots = ISSUE_SLOTS * a.nq * float(a.n_ent) * a.k                     # wave-instructions x 64 lanes
        peak = props.multi_processor_count * 4 * 16 * a.clock_mhz * 1e6  # lanes per second: 4 SIMDs x 16 lanes per CU and cycle
        print("%-8s fast mode    : %9.1f ms  %10.0f ranks/s  (%.2fx)  prefilter %.1f ms (%.0f %% of the VALU issue rate)  re-scoring %.1f ms  "
              "undecided %.3f %%  overflow %d  stats %s"
              % (kind, best["fast"] * 1e3, a.nq / best["fast"], best["exact"] / best["fast"], stage[0], 100.0 * slots / peak / (stage[0] * 1e-3),
                 stage[1], 100.0 * stage[2], stage[3], {k: v for k, v in st.items() if k != "count_ms"}), flush=True)


if __name__ == "__main__":
    main()
