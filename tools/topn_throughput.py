"""Top-N completions at the evaluation shape: ComplEx k=200, |E| = 1M, 8192 query rows, top_n 10 and 100, on random-normal
and on trained-like ("planted": every query's own object aligned with its query vector) tables.  The same run times
emg_eval_count(precision 0) — the same f32 MFMA main loop with the count epilogue — on the same Q and table, and prints the
ratio emg_eval_topn (phase 1 + merge) / emg_eval_count, the queries per second, and once the worst-order cost (scores
increasing with the id).  HIP events on the launch stream, one warm-up, median of 5.  One JSON line per measurement."""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from emgraph_amd import _lib as L  # noqa: E402
from emgraph_amd import device as D  # noqa: E402
from emgraph_amd.training import alloc_table  # noqa: E402

N_ENT, N_REL, K, ROWS = 1_000_000, 1000, 200, 8192
KI = 2 * K
REPS = 5


def timed(fn):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), ms


def main():
    D.require_gpu()
    dev = torch.device("cuda")
    box = "%s, %s" % (torch.cuda.get_device_name(0), L.load().emg_source_hash().decode())
    g = torch.Generator(device=dev).manual_seed(0)
    ent = alloc_table(N_ENT, KI, dev)
    rel = alloc_table(N_REL, KI, dev)
    rs = np.random.RandomState(0)
    T = torch.from_numpy(np.stack([rs.randint(0, N_ENT, ROWS), rs.randint(0, N_REL, ROWS), rs.randint(0, N_ENT, ROWS)], 1).astype(np.int32)).to(dev)
    cnt = torch.zeros((2, ROWS), dtype=torch.int32, device=dev)
    for tables in ("random_normal", "trained_like", "worst_order"):
        with torch.no_grad():
            ent.normal_(0.0, 0.1, generator=g)
            rel.normal_(0.0, 0.1, generator=g)
            Q, pos_int = D.eval_build_queries(L.COMPLEX, ent, rel, KI, 1.0, T, L.EVAL_O)
            if tables == "trained_like":
                b, o = 0.15, T[:, 2].long()
                eo = ent[o]
                qh = Q[:, :KI] / Q[:, :KI].norm(dim=1, keepdim=True)
                ent[o] = (1 - b * b) ** 0.5 * eo + b * eo.norm(dim=1, keepdim=True) * qh
            elif tables == "worst_order":   # entity i scores i * 2^-20 against every query: increasing with the id
                ent.zero_()
                ent[:, 0] = torch.arange(N_ENT, device=dev, dtype=torch.float32) * 2.0 ** -20
                Q.fill_(1.0)
        count_ms, _ = timed(lambda: D.eval_count(L.COMPLEX, Q, pos_int, ent, KI, 1.0, cnt[0], cnt[1]))
        for top_n in ((100,) if tables == "worst_order" else (10, 100)):
            ws = torch.empty(D.eval_topn_ws_bytes(ROWS, N_ENT, top_n), dtype=torch.uint8, device=dev)
            topn_ms, all_ms = timed(lambda: D.eval_topn(L.COMPLEX, Q, ent, KI, 1.0, top_n, ws=ws))
            print(json.dumps({"tool": "topn_throughput", "box": box, "tables": tables, "model": "ComplEx", "k": K, "n_ent": N_ENT,
                              "rows": ROWS, "top_n": top_n, "topn_ms": round(topn_ms, 3), "topn_ms_all": [round(x, 3) for x in all_ms],
                              "count_ms": round(count_ms, 3), "ratio": round(topn_ms / count_ms, 3),
                              "queries_per_s": round(ROWS / (topn_ms * 1e-3)), "ws_mib": ws.numel() >> 20}), flush=True)


if __name__ == "__main__":
    main()
