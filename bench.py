#!/usr/bin/env python3
"""bench.py — BASELINE.json's metric on its own configuration, measured on MI355X.

metric : "positive+negative triples scored/sec at k=200, eta=20; filtered ranks/sec"
workload (N=1 default) : C3 = ComplEx k=200 (k_int=400) eta=20 on synthetic |E|=1M |R|=1k
          (BASELINE.json configs[2]; the config the metric's k=200/eta=20 is quoted on and which
          fits one GPU).  A "step" = one full pass of the hot path over one batch of B positives:
          Philox corruptions -> fused gather+score of B*(1+eta) triples -> NLL loss + dL/dscore
          -> gradients -> deterministic row-sparse SGD apply (the reference forces SGD for
          |E| > 5e5, EmbeddingModel.py:1267-1274).  value = B*(1+eta)*steps*N / time.
          The second half of the metric (filtered ranks/sec, config C4) is reported in "eval".

Contract: W untimed warm-up steps, exactly K timed steps bracketed by barrier + synchronize,
max over ranks, rank 0 prints ONE JSON line.  Inputs are resident in HBM before timing starts
(64 batches of the id-mapped training set; steps cycle over them, one Philox stream per pass).
A plain run does only that (set up, warm up, time, print); --dump-outputs DIR also writes what the
timed steps computed (see dump_outputs).

With --full the line also carries (all measured in the same process, after the timed region):
  sustained : a >= 1 s window of the same step (the K-step window is milliseconds long at the driver's K = 20)
  stages    : per-stage HIP-event times of 16 instrumented steps (instrumentation is OFF in the timed regions)
  roofline  : the dominant byte-moving kernel against the HBM peak
  others    : C3 on Zipf(1.0)-skewed triples, C3 at B = 131072, C3' (TransE k=200 on the 1M table, with the
              gather+score kernel alone), C1, C2, C5 — same step, fewer steps
  eval      : filtered ranks/s (C4): exact f32, bf16 MFMA, query-tile sweep, TransE 1-vs-all
  cpu_baseline : the oracle's C port on the host cores (bounded sample)
"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: HBM3E 8 TB/s (spec)
MFMA_F32_PEAK_TF = 157.3     # f32-input MFMA == f32 vector peak
MFMA_BF16_PEAK_TF = 2500.0   # dense bf16 MFMA (not the 2:1-sparse headline)
N_RESIDENT = 64              # resident batches the steps cycle over

WORKLOADS = {
    # name: model, k, eta, n_ent, n_rel, B, loss, optimizer
    "C3": dict(model="ComplEx", k=200, eta=20, n_ent=1_000_000, n_rel=1000, B=16384, loss="nll", optimizer="sgd",
               desc="ComplEx k=200 (k_int=400) eta=20, synthetic |E|=1M |R|=1k, B=16384/GPU, NLL, SGD"),
    "C3z": dict(model="ComplEx", k=200, eta=20, n_ent=1_000_000, n_rel=1000, B=16384, loss="nll", optimizer="sgd", zipf=True,
                desc="C3 with Zipf(1.0)-skewed subjects/objects (hub entities: hot rows, long segments, few singletons)"),
    "C3b": dict(model="ComplEx", k=200, eta=20, n_ent=1_000_000, n_rel=1000, B=131072, loss="nll", optimizer="sgd",
                desc="C3 at B=131072 (SURVEY 8d's second batch size)", resident=8),
    "C3p": dict(model="TransE", k=200, eta=20, n_ent=1_000_000, n_rel=1000, B=16384, loss="nll", optimizer="sgd",
                desc="C3': TransE-L1 k=200 eta=20 on the |E|=1M table (north_star's HBM-roofline target kernel)"),
    "C3m": dict(model="ComplEx", k=200, eta=20, n_ent=1_000_000, n_rel=1000, B=16384, loss="multiclass_nll", optimizer="sgd",
                desc="C3 with the multiclass-NLL loss (softmax over a positive's negatives: forward | loss | backward kernels)"),
    "C3s": dict(model="ComplEx", k=200, eta=20, n_ent=1_000_000, n_rel=1000, B=16384, loss="self_adversarial", optimizer="sgd",
                desc="C3 with the self-adversarial loss (forward | loss | backward kernels)"),
    "C3r": dict(model="ComplEx", k=200, eta=20, n_ent=1_000_000, n_rel=1000, B=16384, loss="nll", optimizer="sgd",
                reg={"lambda": 1e-5, "p": 2},
                desc="C3 with the LP regulariser (p = 2) folded into the optimizer step (singletons in place in the scoring kernel); the "
                     "dense pass over untouched rows is DEFERRED for tables >= 256 MB (emg_deferred_catchup, same bits)"),
    "C3a": dict(model="ComplEx", k=200, eta=20, n_ent=1_000_000, n_rel=1000, B=16384, loss="nll", optimizer="adam",
                desc="C3 with the reference's default optimizer (Keras Adam, constants.py:55 / adam.py:31-48).  Its update is DENSE — every "
                     "step decays m, v and moves w of all 1M x 400 entries, 9.6 GB read + written.  Default for tables >= 256 MB: the "
                     "decay is DEFERRED (emg_deferred_catchup: the missed steps of a row are replayed when a batch is about to read it — "
                     "same bits, no pass over the whole table)"),
    "C3d": dict(model="ComplEx", k=200, eta=20, n_ent=1_000_000, n_rel=1000, B=16384, loss="nll", optimizer="adam", deferred=False,
                desc="C3a with the dense pass as Keras runs it (Trainer(deferred_dense=False)): every row of the table read and written "
                     "every step"),
    "C3g": dict(model="ComplEx", k=200, eta=20, n_ent=1_000_000, n_rel=1000, B=16384, loss="nll", optimizer="adagrad",
                desc="C3 with Adagrad (row-sparse state: every touched row and its accumulator through the apply kernel)"),
    "C3mo": dict(model="ComplEx", k=200, eta=20, n_ent=1_000_000, n_rel=1000, B=16384, loss="nll", optimizer="momentum",
                 desc="C3 with Keras SGD(momentum): Adagrad's bytes (one state row per touched row) without its sqrt / division — an A/B aid, "
                      "not in `others`"),
    "C2": dict(model="DistMult", k=200, eta=10, n_ent=14541, n_rel=237, B=2722, loss="nll", optimizer="adam",
               desc="DistMult k=200 eta=10 NLL Adam, FB15k-237-shaped, B=2722 (batches_count=100)"),
    "C1": dict(model="TransE", k=100, eta=20, n_ent=38600, n_rel=11, B=1725, loss="pairwise", optimizer="adam",
               desc="TransE-L1 k=100 eta=20 pairwise Adam, WN11-shaped, B=1725 (batches_count=64)"),
    "C5": dict(model="HolE", k=200, eta=20, n_ent=14951, n_rel=1345, B=4832, loss="nll", optimizer="adam",
               desc="HolE k=200 = (2/k) x ComplEx (HolE.py:189; the reference has no FFT HolE, SURVEY A-12) eta=20 NLL Adam, "
                    "FB15k-shaped, B=4832 (batches_count=100)"),
}
MODEL_IDS = {"TransE": 0, "TransE_L2": 1, "DistMult": 2, "ComplEx": 3, "HolE": 4}


def glorot(rs, rows, cols):
    lim = math.sqrt(6.0 / (rows + cols))
    return rs.uniform(-lim, lim, size=(rows, cols)).astype(np.float32)


N_STATE = {"sgd": 0, "momentum": 1, "adagrad": 1, "adam": 2, "adam_lazy": 2}   # optimizer state rows per table row


def algorithmic_bytes(stage, B, eta, k_int, n_unique_ent=None, n_unique_rel=None, n_single=0, ns=0, n_caught_up=0):
    """ALGORITHMIC HBM bytes of one launch (DESIGN.md 'bytes per unit'); int32 ids, fp32 rows.
    n_single: entity slots whose destination is updated IN PLACE by the scoring kernel; ns: optimizer state rows per table row
    (SGD 0, momentum / Adagrad 1, Adam 2) — a row's update reads and writes them with the row."""
    row = 4 * k_int
    if stage == "forward":   # spo + codes + (3+eta) rows + (1+eta) scores
        return B * (12 + 4 * eta + (3 + eta) * row + 4 * (1 + eta))
    if stage == "backward":  # spo + codes + g + (3+eta) rows read + (3+eta) rows written
        return B * (12 + 4 * eta + 4 * (1 + eta) + (3 + eta) * row + (3 + eta) * row)
    if stage == "fused":     # spo + codes + singleton flags + (3+eta) rows read + (3+eta) rows written
        # (a singleton row is written in place — with its ns state rows read and written —, any other row to the contribution buffer)
        return B * (12 + 4 * eta + (2 + eta) + (3 + eta) * row + (3 + eta) * row) + n_single * 2 * ns * row
    if stage == "apply_ent":  # non-singleton contribution rows read once + read-modify-write of each such destination and its state rows
        n_ns = (2 + eta) * B - n_single
        return n_ns * row + 2 * (1 + ns) * (n_unique_ent - n_single) * row + (2 + eta) * B * 8
    if stage == "apply_rel":
        return B * row + 2 * (1 + ns) * n_unique_rel * row + B * 8
    if stage == "catchup":   # deferred dense pass: (w, state) of every destination the apply will finish read, w written back
        return n_caught_up * ((1 + ns) + 1) * row
    return 0


def moved_bytes_model(stage, B, eta, k_int, n_single_neg, n_single_so, n_ns_rows, n_ns_dest):
    """bytes the FACTORED path has to move (bilinear models): a negative's gradient row is one float times
    one of its group's two query rows, so the backward kernel writes 2 query rows + 1 relation row per group, the
    subject / object rows, one float per negative that is not applied in place, and the singleton rows in place."""
    row = 4 * k_int
    if stage == "fused":
        return (B * (12 + 4 * eta + (2 + eta) + (3 + eta) * row)        # ids, codes, flags, rows read
                + B * 3 * row                                             # relation row + the two query rows
                + 2 * B * row                                             # subject / object rows (in place or contribution)
                + n_single_neg * row + (eta * B - n_single_neg) * 4)      # singleton negatives in place; else one float
    if stage == "apply_ent":   # every non-singleton slot reads one (query or kept) row + its factor; RMW of the destination
        return n_ns_rows * (row + 8) + 2 * n_ns_dest * row + (2 + eta) * B * 8
    return 0


def lib_source_hash():
    """hash of the kernel sources libemgraph_hip.so was built from (csrc/build.sh -> emg_source_hash)"""
    try:
        from emgraph_amd import _lib
        return _lib.load().emg_source_hash().decode()
    except Exception:  # noqa: BLE001
        return None


def profile_files(pattern):
    """committed profiles/ files matching `pattern`, newest first by (round number, tag) parsed from r<round>_<tag>_..."""
    import glob
    import re

    def key(fn):
        m = re.match(r"r(\d+)_([A-Za-z0-9]+)_", os.path.basename(fn))
        return (int(m.group(1)), m.group(2)) if m else (-1, "")
    return sorted(glob.glob(os.path.join(ROOT, "profiles", pattern)), key=key, reverse=True)


def pmc_traffic(stage, name, B, world, args):
    """HBM bytes per launch of the dominant kernel from the committed rocprofv3 PMC passes of this command
    (profiles/r2_d_pmc_traffic.json; separate FETCH_SIZE / WRITE_SIZE runs, FETCH_SIZE doubled per MI355X_MICROARCH.md).
    STATIC: read from the file, not measured in this run; only for the configuration it was collected on."""
    if stage != "fused" or name != "C3" or B != 16384 or world != 1 or args.no_inplace or args.no_fused:
        return None, None
    h = lib_source_hash()
    for path in profile_files("r*_pmc_traffic.json"):   # newest round first; only a pass of THIS binary counts
        fn = os.path.basename(path)
        try:
            d = json.load(open(path))
            if d.get("source_hash") != h:
                continue
            k = [v for n, v in d["kernels"].items()
                 if "train_fused_riders_kernel<3, 4, 1, 64, 1>" in n or "train_fused_riders_kernel<3, 4, 1, 64, 1, " in n   # (, window depth> since round 4)
                 or "train_backward_kernel<3, 4, 1, 64, true, 1>" in n]
            if k:
                return k[0]["hbm_bytes_per_launch"], "static: profiles/%s (rocprofv3 --pmc pass of this command and binary %s, not measured in this run)" % (fn, h)
        except (OSError, ValueError, KeyError):
            pass
    return None, "none: no committed rocprofv3 --pmc pass of this binary (source hash %s) under profiles/" % h


def make_triples(w, n, seed):
    rs = np.random.RandomState(seed)
    if w.get("zipf"):   # Zipf(1.0) over a random permutation of the entity ids (hubs are not the low ids)
        wts = 1.0 / np.arange(1, w["n_ent"] + 1)
        perm = rs.permutation(w["n_ent"])
        s, o = perm[rs.choice(w["n_ent"], n, p=wts / wts.sum())], perm[rs.choice(w["n_ent"], n, p=wts / wts.sum())]
    else:
        s, o = rs.randint(0, w["n_ent"], n), rs.randint(0, w["n_ent"], n)
    return np.stack([s, rs.randint(0, w["n_rel"], n), o], 1).astype(np.int32)


class StepRunner:
    """tables + resident batches of one workload; run(n) enqueues n steps cycling over the resident batches"""

    def __init__(self, name, args, rank, world, sharding=None, batch=0):
        import torch

        from emgraph_amd import parallel
        from emgraph_amd.training import Trainer
        self.torch = torch
        w = self.w = WORKLOADS[name]
        self.name = name
        cplx = w["model"] in ("ComplEx", "HolE")
        self.k_full = k_int = 2 * w["k"] if cplx else w["k"]
        self.scale = float(np.float32(2 / w["k"])) if w["model"] == "HolE" else 1.0
        self.B0, self.eta = (batch or w["B"]), w["eta"]
        self.world, self.rank = world, rank
        # weak scaling: the per-GPU batch is fixed, the GLOBAL batch grows with N
        self.B = self.B0 * world
        self.nb = w.get("resident", N_RESIDENT)
        rs = np.random.RandomState(0)  # init seed 0 (constants.py:52)
        self.ent0 = ent0 = glorot(rs, w["n_ent"], k_int)
        self.rel0 = rel0 = glorot(rs, w["n_rel"], k_int)
        self.X = make_triples(w, self.nb * self.B, 1234)  # the SAME triples on every rank
        ent_l, rel_l, self.sharding = ent0, rel0, None
        if world > 1:
            self.sharding = sharding or "k"
            if self.sharding == "k":   # column slabs: every rank walks all B_global groups, 1/N of every row
                ent_l = parallel.shard_columns(ent0, rank, world, cplx)
                rel_l = parallel.shard_columns(rel0, rank, world, cplx)
                k_int = ent_l.shape[1]
        self.k_local = k_int
        self.tr = Trainer(MODEL_IDS[w["model"]], k_int, self.scale, ent_l, rel_l, self.eta, loss=w["loss"],
                          optimizer=w["optimizer"],
                          optimizer_params={"lr": 0.0005}, batches_count=self.nb, seed=0, fused=not args.no_fused,
                          inplace=not args.no_inplace, pipeline=not args.no_pipeline,
                          regularizer="LP" if w.get("reg") else None, regularizer_params=w.get("reg"),
                          deferred_dense=w.get("deferred"),
                          sharded=(self.sharding if self.sharding == "batch" else bool(self.sharding)))
        self.tr.set_training_set(self.X, self.B)
        self.i = 0

    def spec(self, i):
        return ((i % self.nb) * self.B, self.B, i // self.nb + 1, i % self.nb + 1)

    def run(self, n):
        if getattr(self.tr, "graph", False) and self.tr.stage_events is None:   # small batches: graph replays, one call
            self.tr.run_batches([self.spec(self.i + j) for j in range(n)])
            self.i += n
            return
        for _ in range(n):
            i = self.i
            s = self.spec(i)
            self.tr.step(s[0], s[1], epoch=s[2], batch=s[3], prefetch=[self.spec(i + 1), self.spec(i + 2), self.spec(i + 3)])
            self.i += 1

    def sync(self):
        self.torch.cuda.synchronize()
        if self.world > 1:
            self.torch.distributed.barrier()

    def timed(self, n):
        """n steps bracketed by barrier + synchronize; returns (seconds = max over ranks, host enqueue seconds)"""
        torch = self.torch
        self.sync()
        t0 = time.perf_counter()
        self.run(n)
        t_issue = time.perf_counter() - t0
        self.sync()
        dt = time.perf_counter() - t0
        if self.world > 1:
            t = torch.tensor([dt], dtype=torch.float64, device="cuda")
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
            dt = float(t.item())
        return dt, t_issue

    def stages(self, samples=16):
        """per-stage HIP-event times of `samples` instrumented steps + the batch statistics the byte counts need"""
        torch, tr = self.torch, self.tr
        tr.enable_stage_timing(samples)
        self.run(samples)
        ms = {k: float(np.mean(v)) for k, v in tr.stage_times_ms().items()}
        tr.enable_stage_timing(0)
        B, eta = self.B if self.sharding != "batch" else self.B // self.world, self.eta
        out = {}
        n_ce = (2 + eta) * B
        if self.sharding != "batch":
            sl = tr.slots[0]  # any slot holds a full prepared batch of this shape
            n_ue = int(torch.unique(sl["dest_ent"][:n_ce]).numel())
            n_ur = int(torch.unique(sl["dest_rel"][:B]).numel())
            n_single = int(sl["single"][:n_ce].sum().item()) if tr.inplace else 0
            cnt = torch.bincount(sl["dest_ent"][:n_ce].long())
            out["_batch"] = {"unique_ent_rows": n_ue, "singleton_slots": n_single, "unique_rel_rows": n_ur,
                             "longest_segment": int(cnt.max().item()), "segments_over_64_rows": int((cnt > 64).sum().item())}
            ns = N_STATE[self.w["optimizer"]]
            for name, v in ms.items():
                # rows the deferred catch-up brings up to date: every destination of the batch — except the singleton negatives' and
                # singleton s / o rows under Adam's window form, which the scoring kernel replays itself (emg_plan.hip: lag_ip)
                replayed_in_kernel = self.w["optimizer"] == "adam" and getattr(tr, "inplace_mode", 0) == 2
                n_cu = ((n_ue - n_single) if replayed_in_kernel else n_ue) + n_ur
                ab = algorithmic_bytes(name, B, eta, self.k_local, n_ue, n_ur, n_single, ns=ns, n_caught_up=n_cu)
                if name == "apply_ent" and "apply_rel" not in ms:   # pair apply: both tables in the same launches
                    ab += algorithmic_bytes("apply_rel", B, eta, self.k_local, n_ue, n_ur, n_single, ns=ns)
                dense_here = name == "apply_ent" and self.w["optimizer"] == "adam" and not tr.deferred
                if dense_here:   # Keras Adam's dense-equivalent pass: every row the batch did NOT touch is read and written too (w, m, v),
                    ab += ((self.w["n_ent"] - n_ue) + (self.w["n_rel"] - n_ur)) * 2 * (1 + ns) * 4 * self.k_local   # inside this stage's launches
                out[name] = {"ms": round(v, 4), "alg_bytes": ab, "GBps": round(ab / (v * 1e-3) / 1e9, 1) if ab else None}
                if name == "apply_ent" and "apply_rel" not in ms:
                    out[name]["note"] = "entity + relation table through shared launches (emg_apply_grouped_pair)" + (
                        "; bytes include Adam's dense pass over the untouched rows (same launch for tables of <= 131072 rows)" if dense_here else "")
                if name == "catchup":
                    out[name]["note"] = ("emg_deferred_catchup of both tables; bytes = an upper bound (every destination it walks: all of the batch's, "
                                         "minus the singletons Adam's window form replays in the scoring kernel; rows already at the current step "
                                         "— ~30 % at C3 — are skipped)")
                if getattr(tr, "factored", False) and tr.inplace and ns == 0 and name in ("fused", "apply_ent"):
                    flags = sl["single"][:n_ce]
                    n_s_so, n_s_neg = int(flags[:2 * B].sum().item()), int(flags[2 * B:].sum().item())
                    mb = moved_bytes_model(name, B, eta, self.k_local, n_s_neg, n_s_so, n_ce - n_single, n_ue - n_single)
                    out[name]["factored_bytes_model"] = mb
                    out[name]["factored_GBps"] = round(mb / (v * 1e-3) / 1e9, 1)
        else:
            out.update({name: {"ms": round(v, 4)} for name, v in ms.items()})
        return out

    def close(self):
        torch = self.torch
        torch.cuda.synchronize()
        del self.tr
        torch.cuda.empty_cache()


def hbm_ceilings():
    """tools/hbm_ceiling (a standalone HIP program, built by __graft_entry__.build()): what this box's HBM delivers for
    the access mixes of the step — float4 copy, row gather, in-place row read-modify-write, and the fused kernel's own mix
    (23 random 1600-byte rows read per group, 16 written back in place, 5 streamed out).  Run as a child process BEFORE
    the timed region; None if the binary is missing."""
    exe = os.path.join(ROOT, "tools", "hbm_ceiling")
    if not os.path.exists(exe):
        return None
    try:
        out = subprocess.run([exe], capture_output=True, timeout=120, check=True).stdout.decode()
        return json.loads(out)
    except (subprocess.SubprocessError, ValueError, OSError):
        return None


def profiled_avg_us(kernel_substr, tag_glob="r*_c3_kernel_stats.md"):
    """average duration (us) of a kernel in the newest committed rocprofv3 --kernel-trace --stats table of THIS workload
    (profiles/): printed next to the live HIP-event figure so that `frac` can be re-derived from profiles/ alone"""
    h = lib_source_hash()
    for fn in profile_files(tag_glob):   # newest first; only a table of THIS binary (its first line names the source hash)
        lines = open(fn).read().splitlines()
        if not lines or ("source_hash: %s" % h) not in lines[0]:
            continue
        for line in lines:
            if kernel_substr in line and line.startswith("|"):
                cells = [c.strip() for c in line.strip().strip("|").split("|")]
                try:
                    return {"file": "profiles/" + os.path.basename(fn), "kernel": cells[0], "calls": int(cells[1]), "avg_us": float(cells[3]),
                            "min_us": float(cells[4]), "source_hash": h}
                except (ValueError, IndexError):
                    pass
                break
    return None


def copy_rate(torch):
    """on-box streaming-copy rate (1 GiB read + 1 GiB written per copy): the practical HBM ceiling next to the
    8 TB/s datasheet peak (SURVEY 8d asks for both denominators)"""
    src = torch.empty(1 << 28, dtype=torch.float32, device="cuda")
    dst = torch.empty_like(src)
    dst.copy_(src)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        dst.copy_(src)
    e1.record()
    torch.cuda.synchronize()
    return 5 * 2 * src.numel() * 4 / (e0.elapsed_time(e1) * 1e-3) / 1e9


DUMP_ENT_SAMPLE = 8192       # seeded sample of entity rows written by --dump-outputs
DUMP_ENT_BATCH = 2048        # positives of the last timed batch whose subject / object rows are written


def dump_outputs(r, loss, out_dir, write):
    """What the timed path hands its caller after the last timed step: the updated tables (a fixed sample of the entity
    table's rows — the subjects / objects of the first DUMP_ENT_BATCH positives of the last timed batch, then
    DUMP_ENT_SAMPLE rows drawn with seed 0 — and the whole relation table) and the loss summed over the warm-up and timed
    steps.  float32 tables, float64 loss; 21 MB at C3.  With N > 1 ranks: rank 0's tables (its column slab under k-sharding).
    Every rank brings deferred rows up to date (local kernels only); `write` (rank 0) writes the files."""
    tr = r.tr
    tr.materialize()                          # deferred dense pass (Adam / LP regulariser on large tables): rows as a caller reads them
    start, B = r.spec(r.i - 1)[:2]            # the last step run
    pos = r.X[start:start + min(B, DUMP_ENT_BATCH)]
    batch_rows = np.stack([pos[:, 0], pos[:, 2]], 1).reshape(-1).astype(np.int64)
    sample_rows = np.sort(np.random.RandomState(0).choice(r.w["n_ent"], min(DUMP_ENT_SAMPLE, r.w["n_ent"]), replace=False))
    idx = r.torch.from_numpy(np.concatenate([batch_rows, sample_rows])).to(tr.ent.device)
    ent_rows = tr.ent.index_select(0, idx).cpu().numpy()
    rel = tr.rel.cpu().numpy()
    if not write:
        return
    os.makedirs(out_dir, exist_ok=True)
    nb = len(batch_rows)
    arrays = {"ent_rows_last_batch": ent_rows[:nb], "ent_rows_sample": ent_rows[nb:], "rel_table": rel,
              "loss_sum": np.array([loss], dtype=np.float64)}
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a))


def step_summary(r, dt, t_issue, steps):
    return {"value": round(r.B * (1 + r.eta) * steps / dt, 1), "unit": "triples scored/s", "steps": steps,
            "seconds": round(dt, 4), "ms_per_step": round(dt / steps * 1e3, 4),
            "host_issue_ms_per_step": round(t_issue / steps * 1e3, 4)}


def score_kernel_alone(r, reps=50):
    """the gather+score kernel by itself (emg_train_forward: positives + eta negatives per group, scores written):
    HIP events over `reps` back-to-back launches on the current stream"""
    import torch

    from emgraph_amd import _lib as L
    from emgraph_amd import device as D
    tr = r.tr
    B, eta = r.B, r.eta
    pos = tr.X[:B]
    codes = D.corrupt_codes(B, eta, L.SIDE_SO, r.w["n_ent"], "cuda", seed=0, counter=12345)
    sp = torch.empty(B, dtype=torch.float32, device="cuda")
    sn = torch.empty(B * eta, dtype=torch.float32, device="cuda")
    for _ in range(3):
        D.train_forward(tr.model_id, tr.ent, tr.rel, tr.k_int, tr.scale, pos, eta, codes, scores_pos=sp, scores_neg=sn)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        D.train_forward(tr.model_id, tr.ent, tr.rel, tr.k_int, tr.scale, pos, eta, codes, scores_pos=sp, scores_neg=sn)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    ab = algorithmic_bytes("forward", B, eta, tr.k_int)
    traffic, fn = None, None
    try:
        for path in profile_files("r*_pmc_traffic.json"):
            d = json.load(open(path))
            if d.get("source_hash") != lib_source_hash():
                continue
            k = [v for n, v in d["kernels"].items() if "train_forward_kernel<0, 4, 1, 64>" in n and "16384 groups" in n]
            if k:
                traffic, fn = k[0]["hbm_bytes_per_launch"], os.path.basename(path)
                break
    except (OSError, ValueError, KeyError):
        pass
    return {"kernel": "train_forward_kernel (gather + score of %d x %d triples)" % (B, 1 + eta), "bound": "hbm",
            "avg_launch_ms": round(ms, 4), "alg_bytes_per_launch": ab, "achieved": round(ab / (ms * 1e-3) / 1e9, 1),
            "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ab / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
            "traffic": traffic, "traffic_source": ("static: profiles/" + fn) if traffic else None,
            "triples_per_s": round(B * (1 + eta) / (ms * 1e-3), 1)}


def run_eval(r, args):
    """C4: filtered 1-vs-all ranks/sec on trained-scale tables ('s+o', worst)"""
    import torch

    from emgraph_amd import device as D
    from emgraph_amd import parallel
    from emgraph_amd.evaluation import FilterIndex, rank_triples_device
    from emgraph_amd.training import alloc_table
    w = r.w
    rank, world = parallel.rank_world()
    n_test = args.eval_triples
    rs = np.random.RandomState(99)
    T = r.X[rs.choice(len(r.X), n_test, replace=False)]
    F = FilterIndex(r.X)  # one-off index of the filter triples (not timed: built once per evaluation run)
    mid = MODEL_IDS[w["model"]]
    k_int = r.k_full
    # trained-scale tables (N(0, 0.1)): the Glorot start values are ~1e-3, whose scores all truncate to the
    # same int32(score*1e5) — legal but unrepresentative of a ranking workload
    ers = np.random.RandomState(7)
    dev = torch.device("cuda")
    ent = alloc_table(w["n_ent"], k_int, dev, init=(ers.randn(w["n_ent"], k_int) * 0.1).astype(np.float32))
    rel = alloc_table(w["n_rel"], k_int, dev, init=(ers.randn(w["n_rel"], k_int) * 0.1).astype(np.float32))
    shard = (rank, world) if world > 1 else None
    n_ranks = 2 * n_test  # one rank = one (test triple, side)
    flops = 2.0 * k_int * w["n_ent"] * n_ranks
    kflops = flops / world  # each rank's count kernels cover its candidate range

    def timed(T_, **kw):
        # untimed warm-up on enough triples (> 128 query rows) to take the same kernels as the timed call: a kernel's first
        # launch loads its code object and sets its LDS attribute (~30 ms once per process for the prefilter + re-scoring pair)
        # (half of the test set: long enough segments for the segment-wise re-scoring kernel too — with 192 triples it was sometimes
        # first launched inside the timed call: 164 k instead of 406 k ranks/s in one run of round 4)
        # (precision 2: the WHOLE test set — its pair buffer is sized by the call, 1 GiB at 8192 query rows x 1M entities, and a
        # half-size warm-up left that allocation inside the timed call: 180 k instead of 530 k ranks/s in one run of round 6)
        warm = T_ if kw.get("precision") == 2 else T_[:max(192, len(T_) // 2)]
        rank_triples_device(mid, ent, rel, k_int, r.scale, warm, "s+o", "worst", filter_triples=F, shard=shard, **kw)
        torch.cuda.synchronize()
        if world > 1:
            torch.distributed.barrier()
        st = {}
        t0 = time.perf_counter()
        rk = rank_triples_device(mid, ent, rel, k_int, r.scale, T_, "s+o", "worst", filter_triples=F, shard=shard, stats=st, **kw)
        torch.cuda.synchronize()
        return rk, time.perf_counter() - t0, st

    ranks, dt, st = timed(T)
    out = {"metric": "filtered ranks/sec", "value": round(n_ranks / dt, 1), "unit": "ranks/s", "test_triples": n_test,
           "corrupt_side": "s+o", "precision": "f32 (exact, v_mfma_f32_32x32x2_f32)", "seconds": round(dt, 4),
           "mean_rank": float(np.mean(ranks))}
    kt = st["count_ms"] * 1e-3
    out["roofline"] = {"bound": "mfma", "kernel": "count_mfma_pipe_kernel", "achieved": round(kflops / kt / 1e12, 2),
                       "peak": MFMA_F32_PEAK_TF, "unit": "TFLOP/s", "frac": round(kflops / kt / 1e12 / MFMA_F32_PEAK_TF, 4),
                       "launches": st["count_launches"], "kernel_ms": round(st["count_ms"], 3),
                       "end_to_end_TFLOPs": round(flops / dt / 1e12, 2),
                       "note": "kernel time from HIP events around the count launches; end-to-end adds query build, "
                               "filter CSR + H2D, filter kernel, D2H; f32-input MFMA peak"}
    # bf16 MFMA throughput mode (statistical rank agreement); the bf16 copy of the table is made once per
    # evaluation run, like the filter index
    eb = D.to_bf16(ent, k_int, ld_dst=D.bf16_ld(k_int))
    rb, dtb, stb = timed(T, precision=1, ent_bf16=eb)
    ktb = stb["count_ms"] * 1e-3
    out["bf16"] = {"value": round(n_ranks / dtb, 1), "unit": "ranks/s", "seconds": round(dtb, 4),
                   "precision": "bf16 operands, f32 accumulate (v_mfma_f32_32x32x16_bf16)",
                   "median_rel_rank_error_vs_exact": float(np.median(np.abs(rb - ranks) / (2.0 * w["n_ent"]))),
                   "roofline": {"bound": "mfma", "kernel": "count_mfma_bf16_v4_kernel<25,1> (one counter: 64 query rows per wave; v3 with two counters)",
                                "achieved": round(kflops / ktb / 1e12, 2), "peak": MFMA_BF16_PEAK_TF,
                                "unit": "TFLOP/s", "frac": round(kflops / ktb / 1e12 / MFMA_BF16_PEAK_TF, 4),
                                "launches": stb["count_launches"], "kernel_ms": round(stb["count_ms"], 3),
                                "end_to_end_TFLOPs": round(flops / dtb / 1e12, 2)}}
    # precision 2: EXACT ranks (bit-equal to the f32 path, asserted here) through the half-precision MFMA prefilter +
    # exact re-scoring of the candidates inside the rigorous error band.  Two data sets: the random positives above
    # (mean rank ~ |E|/2: the most undecided candidates a Gaussian table can produce, ~0.7 %) and PLANTED positives
    # (each test object's row pulled towards its query so that it scores ~3.3 sigma: ranks in the top ~0.1 %, what a
    # trained model's evaluation looks like)
    from emgraph_amd.evaluation import PrefilterTables
    tabs = PrefilterTables(ent, k_int)
    ex = {}
    for label in ("random_positives", "planted_positives"):
        if label == "planted_positives":
            Q1, _ = D.eval_build_queries(mid, ent, rel, k_int, r.scale, torch.from_numpy(T).to(dev), 1)
            o = torch.from_numpy(T[:, 2].astype(np.int64)).to(dev)
            qh = Q1[:, :k_int] / Q1[:, :k_int].norm(dim=1, keepdim=True)
            ent[o] = (1 - 0.15 ** 2) ** 0.5 * ent[o] + 0.15 * ent[o].norm(dim=1, keepdim=True) * qh
            tabs = PrefilterTables(ent, k_int)
            ranks, dt, st = timed(T)
        rf, dtf, stf = timed(T, precision=2, ent_f16=tabs)
        assert np.array_equal(rf, ranks), "precision 2 ranks differ from the exact path"
        ex[label] = {"value": round(n_ranks / dtf, 1), "unit": "ranks/s", "seconds": round(dtf, 4), "mean_rank": float(np.mean(rf)),
                     "equal_to_exact_f32_ranks": True, "exact_f32_ranks_per_s": round(n_ranks / dt, 1),
                     "undecided_pairs": stf.get("pairs", 0), "undecided_fraction": round(stf.get("pairs", 0) / (n_ranks * w["n_ent"] / world), 6),
                     "tiles_redone_by_exact_kernel": stf.get("fallback", 0), "kernel_ms": round(stf["count_ms"], 3),
                     # the contraction's flops over ALL the mode's kernels (prefilter + compaction + re-scoring): the fraction of the
                     # half-precision dense peak at which this parity-exact mode delivers the 1-vs-all product
                     "mfma_frac_all_kernels": round(kflops / (stf["count_ms"] * 1e-3) / 1e12 / MFMA_BF16_PEAK_TF, 4),
                     "kernels": "count_mfma_bf16_v4_kernel<25,3> (v_mfma_f32_32x32x16_f16, transposed products, undecided candidates as a bitmap) + prefilter_compact_kernel + rescore_segment_kernel (segments of >= 512 pairs: query rows in LDS) / rescore_pairs_kernel"}
    # a FRESH model (round 6): Glorot-scale tables (limit 2.45e-3 at 1M x 400) — every score truncates to the comparison integer 0, every
    # candidate ties with the positive; the prefilter's second form proves the ties (emg_eval_prefilter_f16_ties), the plain form could
    # only hand the whole tile to the exact kernel.  What early stopping's first evaluations and a one-epoch model see.
    fresh_e = alloc_table(w["n_ent"], k_int, dev, init=None)
    fresh_r = alloc_table(w["n_rel"], k_int, dev, init=None)
    with torch.no_grad():
        fresh_e.uniform_(-2.45e-3, 2.45e-3, generator=torch.Generator(device=dev).manual_seed(11))
        fresh_r.uniform_(-7.7e-2, 7.7e-2, generator=torch.Generator(device=dev).manual_seed(12))
    ent_keep, rel_keep = ent, rel
    ent, rel = fresh_e, fresh_r
    try:
        rx, dtx, stx = timed(T)
        rt_, dtt, stt = timed(T, precision=2, ent_f16=PrefilterTables(ent, k_int))
        assert np.array_equal(rt_, rx), "precision 2 ranks differ from the exact path on the fresh table"
        ex["fresh_model"] = {"value": round(n_ranks / dtt, 1), "unit": "ranks/s", "seconds": round(dtt, 4), "equal_to_exact_f32_ranks": True,
                             "exact_f32_ranks_per_s": round(n_ranks / dtx, 1), "proved_ties": bool(stt.get("prove_ties")),
                             "tiles_redone_by_exact_kernel": stt.get("fallback", 0), "undecided_pairs": stt.get("pairs", 0),
                             "kernel_ms": round(stt["count_ms"], 3),
                             "kernels": "count_mfma_bf16_v3_kernel<25,4,4> (four thresholds per row: greater | proven tie | the two bands) + prefilter_compact_kernel + rescore_pairs_kernel"}
    finally:
        ent, rel = ent_keep, rel_keep
        del fresh_e, fresh_r
    # what the API call pays when nothing is cached (get_ranks / early stopping pass no tables: the half-precision copy, the
    # norm bounds and the range are rebuilt inside the call) — the figures above build them once per evaluation run, outside
    ru, dtu, _ = timed(T, precision=2)
    assert np.array_equal(ru, ranks)
    ex["planted_positives"]["uncached_tables"] = {"value": round(n_ranks / dtu, 1), "unit": "ranks/s", "seconds": round(dtu, 4),
                                                  "note": "same call with ent_f16=None: the derived tables are rebuilt inside the timed region"}
    out["exact_fast"] = ex
    out["product_default"] = ("evaluate_performance / get_ranks pick precision 'auto': the exact_fast path (bit-equal ranks) for "
                              "DistMult / ComplEx / HolE at k_int in 33..800 and (transe_l1.exact_fast, transe_l2.exact_fast) for TransE-L1 (any k) and TransE-L2 (k + 2 <= 800), "
                              ">= 128 test triples, >= 32768 entities, no candidate subset; the exact f32 kernel (`value`) otherwise")
    if not args.quick:
        # query-tile sweep (B_q in {128, 512, 2048} query rows per pass over the table), bf16 mode
        sweep = {}
        for bq in (128, 512, 2048):
            Tq = T[:1024]            # 2048 query rows: 16 / 4 / 1 passes over the table
            _, dq, sq = timed(Tq, precision=1, ent_bf16=eb, query_chunk=bq // 2)
            nr = 2 * len(Tq)
            sweep["B_q=%d" % bq] = {"ranks_per_s": round(nr / dq, 1), "kernel_ms_per_pass": round(sq["count_ms"] / sq["count_launches"], 3),
                                    "MFMA_frac": round(2.0 * k_int * w["n_ent"] * nr / world / (sq["count_ms"] * 1e-3) / 1e12 / MFMA_BF16_PEAK_TF, 4)}
        out["bf16"]["query_tile_sweep"] = sweep
        # TransE-L1 1-vs-all (not a contraction: LDS-tiled f32 VALU kernel), k=200 on the same number of entities
        kt_ = 200
        ent_t = alloc_table(w["n_ent"], kt_, dev, init=(ers.randn(w["n_ent"], kt_) * 0.1).astype(np.float32))
        rel_t = alloc_table(w["n_rel"], kt_, dev, init=(ers.randn(w["n_rel"], kt_) * 0.1).astype(np.float32))
        Tt = T[:512]
        rank_triples_device(0, ent_t, rel_t, kt_, 1.0, Tt[:32], "s+o", "worst", filter_triples=F, shard=shard)
        torch.cuda.synchronize()
        stt = {}
        t0 = time.perf_counter()
        rank_triples_device(0, ent_t, rel_t, kt_, 1.0, Tt, "s+o", "worst", filter_triples=F, shard=shard, stats=stt)
        torch.cuda.synchronize()
        dtt = time.perf_counter() - t0
        lane_ops = 2.0 * kt_ * w["n_ent"] * 2 * len(Tt) / world   # one subtract + one |.|-accumulate per (row, entity, k)
        out["transe_l1"] = {"value": round(2 * len(Tt) / dtt, 1), "unit": "ranks/s", "test_triples": len(Tt), "k": kt_,
                            "kernel": "count_transe_big_kernel (f32 VALU, 128x128 tiles, 8x8 per thread)", "kernel_ms": round(stt["count_ms"], 3),
                            "roofline": {"bound": "valu", "achieved": round(lane_ops / (stt["count_ms"] * 1e-3) / 1e12, 2),
                                         "peak": MFMA_F32_PEAK_TF / 2, "unit": "T lane-op/s (f32 VALU: 157.3 TFLOP/s counts an FMA as 2)",
                                         "frac": round(lane_ops / (stt["count_ms"] * 1e-3) / 1e12 / (MFMA_F32_PEAK_TF / 2), 4)}}
        # the same ranks through the fixed-point prefilter (v_sad_u16: two coordinates per instruction) + exact re-scoring
        from emgraph_amd.evaluation import SadTables
        exact_t = rank_triples_device(0, ent_t, rel_t, kt_, 1.0, Tt, "s+o", "worst", filter_triples=F, shard=shard)
        tabs = SadTables(ent_t, rel_t, kt_)
        rank_triples_device(0, ent_t, rel_t, kt_, 1.0, Tt[:32], "s+o", "worst", filter_triples=F, shard=shard, precision=2, ent_f16=tabs)
        torch.cuda.synchronize()
        sts = {}
        t0 = time.perf_counter()
        fast_t = rank_triples_device(0, ent_t, rel_t, kt_, 1.0, Tt, "s+o", "worst", filter_triples=F, shard=shard, precision=2,
                                     ent_f16=tabs, stats=sts)
        torch.cuda.synchronize()
        dts = time.perf_counter() - t0
        sad_ops = ((kt_ + 15) // 16 * 8) * float(w["n_ent"]) * 2 * len(Tt) / world    # v_sad_u16 lane-instructions (k padded to 16)
        valu_issue_peak = 256 * 4 * 16 * 2.4e9 / 1e12                                  # one VALU instruction per SIMD and 4 clocks
        out["transe_l1"]["exact_fast"] = {
            "value": round(2 * len(Tt) / dts, 1), "unit": "ranks/s", "equal_to_exact_f32_ranks": bool(np.array_equal(fast_t, exact_t)),
            "undecided_pairs": int(sts.get("pairs", 0)), "undecided_fraction": round(sts.get("pairs", 0) / (2.0 * len(Tt) * w["n_ent"] / world), 6),
            "tiles_redone_by_exact_kernel": int(sts.get("fallback", 0)), "kernel_ms": round(sts["count_ms"], 3),
            "kernels": "count_sad_kernel (v_sad_u16 over 16-bit fixed-point images) + rescore_pairs_kernel",
            "roofline": {"bound": "valu", "achieved": round(sad_ops / (sts["count_ms"] * 1e-3) / 1e12, 2), "peak": round(valu_issue_peak, 2),
                         "unit": "T lane-instr/s (VALU issue rate; kernel_ms includes the re-scoring)",
                         "frac": round(sad_ops / (sts["count_ms"] * 1e-3) / 1e12 / valu_issue_peak, 4)}}
        # TransE-L2: exact f32 VALU kernel, and the same ranks through the MFMA prefilter on the augmented rows
        from emgraph_amd.evaluation import L2Tables
        T2 = T[:1024]
        rank_triples_device(1, ent_t, rel_t, kt_, 1.0, T2[:32], "s+o", "worst", filter_triples=F, shard=shard)
        torch.cuda.synchronize()
        st2 = {}
        t0 = time.perf_counter()
        exact_2 = rank_triples_device(1, ent_t, rel_t, kt_, 1.0, T2, "s+o", "worst", filter_triples=F, shard=shard, stats=st2)
        torch.cuda.synchronize()
        dt2 = time.perf_counter() - t0
        tabs2 = L2Tables(ent_t, kt_)
        rank_triples_device(1, ent_t, rel_t, kt_, 1.0, T2[:160], "s+o", "worst", filter_triples=F, shard=shard, precision=2, ent_f16=tabs2)
        torch.cuda.synchronize()
        st3 = {}
        t0 = time.perf_counter()
        fast_2 = rank_triples_device(1, ent_t, rel_t, kt_, 1.0, T2, "s+o", "worst", filter_triples=F, shard=shard, precision=2,
                                     ent_f16=tabs2, stats=st3)
        torch.cuda.synchronize()
        dt3 = time.perf_counter() - t0
        mfma_flops = 2.0 * 208 * w["n_ent"] * 2 * len(T2) / world     # k + 2 = 202 coordinates in 13 k-steps of 16
        out["transe_l2"] = {
            "value": round(2 * len(T2) / dt2, 1), "unit": "ranks/s", "test_triples": len(T2), "k": kt_,
            "kernel": "count_transe_big_kernel<L2> (f32 VALU)", "kernel_ms": round(st2["count_ms"], 3),
            "exact_fast": {
                "value": round(2 * len(T2) / dt3, 1), "unit": "ranks/s", "equal_to_exact_f32_ranks": bool(np.array_equal(fast_2, exact_2)),
                "undecided_pairs": int(st3.get("pairs", 0)), "undecided_fraction": round(st3.get("pairs", 0) / (2.0 * len(T2) * w["n_ent"] / world), 6),
                "tiles_redone_by_exact_kernel": int(st3.get("fallback", 0)), "kernel_ms": round(st3["count_ms"], 3),
                "kernels": "count_mfma_bf16_v4_kernel<13,3> (v_mfma_f32_32x32x16_f16 over [2q|-1|-1].[e|n_hi|n_lo], bitmap form) + prefilter_compact_kernel + rescore_pairs_kernel",
                "roofline": {"bound": "mfma", "achieved": round(mfma_flops / (st3["count_ms"] * 1e-3) / 1e12, 1), "peak": MFMA_BF16_PEAK_TF,
                             "unit": "TFLOP/s (kernel_ms includes the re-scoring)",
                             "frac": round(mfma_flops / (st3["count_ms"] * 1e-3) / 1e12 / MFMA_BF16_PEAK_TF, 4)}}}
        # ComplEx k = 400 (k_int = 800): the 4-wave form of the prefilter (128 query rows per workgroup, up to 50 query
        # fragments in one wave's 512 registers), positives planted near the top as above
        del ent_t, rel_t
        kw_ = 800
        ent_w = alloc_table(w["n_ent"], kw_, dev, init=None)
        rel_w = alloc_table(w["n_rel"], kw_, dev, init=None)
        g = torch.Generator(device=dev); g.manual_seed(7)
        ent_w[:, :kw_] = torch.randn(w["n_ent"], kw_, device=dev, generator=g) * 0.1
        rel_w[:, :kw_] = torch.randn(w["n_rel"], kw_, device=dev, generator=g) * 0.1
        Tw = T[:1024]
        Qw, _ = D.eval_build_queries(3, ent_w, rel_w, kw_, 1.0, torch.from_numpy(Tw).to(dev), 1)
        ow = torch.from_numpy(Tw[:, 2].astype(np.int64)).to(dev)
        qh = Qw[:, :kw_] / Qw[:, :kw_].norm(dim=1, keepdim=True)
        ent_w[ow] = (1 - 0.15 ** 2) ** 0.5 * ent_w[ow] + 0.15 * ent_w[ow].norm(dim=1, keepdim=True) * qh
        from emgraph_amd.evaluation import PrefilterTables
        tabs_w = PrefilterTables(ent_w, kw_)
        res_w = {}
        for prec, kwargs in ((0, {}), (2, dict(ent_f16=tabs_w))):
            rank_triples_device(3, ent_w, rel_w, kw_, 1.0, Tw[:192], "s+o", "worst", filter_triples=F, shard=shard, precision=prec, **kwargs)
            torch.cuda.synchronize()
            stw = {}
            t0 = time.perf_counter()
            rw = rank_triples_device(3, ent_w, rel_w, kw_, 1.0, Tw, "s+o", "worst", filter_triples=F, shard=shard, precision=prec, stats=stw, **kwargs)
            torch.cuda.synchronize()
            res_w[prec] = (rw, time.perf_counter() - t0, stw)
        out["complex_k400"] = {
            "value": round(2 * len(Tw) / res_w[0][1], 1), "unit": "ranks/s", "test_triples": len(Tw), "k_int": kw_,
            "kernel": "count_mfma_pipe_kernel (exact f32)", "kernel_ms": round(res_w[0][2]["count_ms"], 3),
            "exact_fast": {"value": round(2 * len(Tw) / res_w[2][1], 1), "unit": "ranks/s",
                           "equal_to_exact_f32_ranks": bool(np.array_equal(res_w[0][0], res_w[2][0])),
                           "undecided_pairs": int(res_w[2][2].get("pairs", 0)), "tiles_redone_by_exact_kernel": int(res_w[2][2].get("fallback", 0)),
                           "kernel_ms": round(res_w[2][2]["count_ms"], 3), "mean_rank": float(np.mean(res_w[2][0])),
                           "kernels": "count_mfma_bf16_v3_kernel<50,4,3,4> (4 waves x 128 query rows, bitmap form) + prefilter_compact_kernel + rescore_segment_kernel<0,4> / rescore_pairs_kernel"}}
    return out


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(r, args):
    """The CPU baseline: oracle/emg_cpu_fast.c — an OPTIMISED C/OpenMP forward pass (hoisted query vectors, SIMD
    reductions, software prefetch; rebuilt with -march=native on this host) — on all host cores over a bounded sample of
    the same workload: forward scoring of B*(1+eta) triples per batch.  A reported baseline, not the target.  The
    order-pinned bit-exactness checker (emg_oracle.c, -O2 -ffp-contract=off) is timed beside it for reference."""
    from oracle import c_oracle as co
    w = r.w
    B, eta, k_int = r.B, r.eta, r.k_full
    mid = MODEL_IDS[w["model"]]
    X = r.X
    nb = max(1, min(args.cpu_batches, len(X) // B))
    co.lib()
    codes = [co.corrupt_codes(B, eta, 2, w["n_ent"], 0, i) for i in range(nb)]

    def timed(fn, seconds):
        fn(mid, r.ent0, r.rel0, k_int, r.scale, X[:256], eta, codes[0][:256 * eta])  # warm
        t0 = time.perf_counter()
        done = 0
        while True:  # cycle over the sample's batches until ~seconds of CPU work has been timed
            for i in range(nb):
                fn(mid, r.ent0, r.rel0, k_int, r.scale, X[i * B:(i + 1) * B], eta, codes[i])
            done += nb
            if time.perf_counter() - t0 >= seconds:
                break
        return done, time.perf_counter() - t0

    done, dt = timed(co.fast_train_forward, args.cpu_seconds)
    fast = co.fast_lib()
    out = {"value": round(done * B * (1 + eta) / dt, 1), "unit": "triples scored/s", "cores": int(fast.cpufast_num_threads()),
           "kind": "port", "cpu": cpu_model(),
           "build": os.path.basename(fast._so) + (" (-O3 -march=native, omp simd)" if "native" in fast._so else " (-O3 -march=x86-64-v3, omp simd)"),
           "sample": "%d passes over %d batches of B=%d (%d triples scored), optimised C/OpenMP gather+score (forward only: "
           "hoisted query vectors, SIMD reductions, prefetch), same tables" % (done // nb, nb, B, done * B * (1 + eta)),
           "seconds": round(dt, 3)}
    done2, dt2 = timed(co.train_forward, min(3.0, args.cpu_seconds))
    out["bit_exact_checker"] = {"value": round(done2 * B * (1 + eta) / dt2, 1), "unit": "triples scored/s",
                                "note": "oracle/emg_oracle.c (order-pinned scalar reduction, -O2 -ffp-contract=off): the parity checker, "
                                        "not a performance baseline", "seconds": round(dt2, 3)}
    # the literal op-by-op numpy restatement (3 materialised gathers + elementwise passes, one
    # thread) — the closest stand-in for the reference's TF-eager-CPU graph; bounded to ~2e5 triples
    from oracle import emgraph_oracle as orc
    Bs = min(B, 8192)
    xp = X[:Bs]
    xn = orc.generate_corruptions_for_fit_philox(xp, eta=eta, corrupt_side="s,o", entities_size=w["n_ent"], seed=0, counter=0)
    kk = w["k"]
    t0 = time.perf_counter()
    orc.score_triples(w["model"], r.ent0, r.rel0, xp, k=kk)
    orc.score_triples(w["model"], r.ent0, r.rel0, xn, k=kk)
    dtn = time.perf_counter() - t0
    out["numpy_unfused_1thread"] = {"value": round(Bs * (1 + eta) / dtn, 1), "unit": "triples scored/s",
                                    "sample": "%d triples scored" % (Bs * (1 + eta)), "seconds": round(dtn, 3)}
    return out


SUMMARY_MAX_BYTES = 4096
DETAIL_FILE = "bench_detail.json"


def _finite(x):
    """strict JSON has no NaN / Infinity: non-finite floats become null (recursively)"""
    if isinstance(x, float):
        return x if math.isfinite(x) else None
    if isinstance(x, dict):
        return {str(k): _finite(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_finite(v) for v in x]
    if isinstance(x, (np.floating, np.integer)):
        return _finite(x.item())
    if isinstance(x, np.bool_):
        return bool(x)
    return x


def _pick(d, *keys):
    return {k: d[k] for k in keys if isinstance(d, dict) and k in d}


def summary_line(line, detail_file=DETAIL_FILE):
    """The ONE stdout line of the contract, <= SUMMARY_MAX_BYTES of strict JSON, built from the full result `line` (which goes to
    `detail_file`): the contract's keys, the dominant kernel's roofline, the default-optimizer block, ranks/s of the three
    evaluation modes, ms/step of the secondary workloads and the CPU baseline — numbers only, no prose."""
    s = _pick(line, "metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data")
    cfg = line.get("config", {})
    s["config"] = dict(_pick(cfg, "B_per_gpu", "global_batch", "eta", "k_int", "k_int_per_gpu", "n_ent", "n_rel"),
                       workload=str(cfg.get("workload", ""))[:120], parallelism=str(cfg.get("parallelism", ""))[:80])
    if "sustained" in line:
        s["sustained"] = _pick(line["sustained"], "value", "ms_per_step", "steps")
    st = line.get("stages", {})
    s["stages_ms"] = {k: v["ms"] for k, v in st.items() if isinstance(v, dict) and "ms" in v}
    rf = line.get("roofline")
    if rf:
        r = _pick(rf, "kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "alg_bytes_per_launch", "avg_launch_ms")
        r["traffic_source"] = (rf.get("traffic_source") or None) and str(rf["traffic_source"])[:72]
        if "profiled" in rf:
            r["profiled"] = _pick(rf["profiled"], "file", "avg_us", "frac")
        if "mix_ceiling" in rf:
            r["mix_ceiling_ms"] = rf["mix_ceiling"].get("ms")
        s["roofline"] = r
    do = line.get("default_optimizer")
    if do:
        s["default_optimizer"] = dict(_pick(do, "value", "ms_per_step", "steps", "stages_ms"), workload="C3a: C3 with Keras Adam (the reference's default)",
                                      roofline=_pick(do.get("roofline", {}), "kernel", "frac", "achieved", "alg_bytes_per_launch", "avg_launch_ms"))
    if "others" in line:
        s["others_ms_per_step"] = {k: v.get("ms_per_step") for k, v in line["others"].items()}
    ev = line.get("eval")
    if ev:
        e = {"unit": "ranks/s", "test_triples": ev.get("test_triples"),
             "exact": {"value": ev.get("value"), "frac": ev.get("roofline", {}).get("frac"), "peak_TF": MFMA_F32_PEAK_TF}}
        if "bf16" in ev:
            b = ev["bf16"]
            e["bf16"] = {"value": b.get("value"), "frac": b.get("roofline", {}).get("frac"), "peak_TF": MFMA_BF16_PEAK_TF}
            sw = b.get("query_tile_sweep")
            if sw:
                e["bf16"]["frac_by_query_tile"] = {k.replace("B_q=", ""): v.get("MFMA_frac") for k, v in sw.items()}
        for label, short in (("random_positives", "exact_fast_random"), ("planted_positives", "exact_fast_planted"), ("fresh_model", "exact_fast_fresh")):
            x = ev.get("exact_fast", {}).get(label)
            if x:
                e[short] = _pick(x, "value", "equal_to_exact_f32_ranks", "undecided_fraction", "kernel_ms", "mfma_frac_all_kernels", "exact_f32_ranks_per_s", "proved_ties")
        s["eval"] = e
    cpu = line.get("cpu_baseline")
    if cpu:
        s["cpu_baseline"] = dict(_pick(cpu, "value", "unit", "cores", "kind", "cpu", "seconds"), scope=cpu.get("scope", "forward only"),
                                 sample=str(cpu.get("sample", ""))[:160])
    for k in ("xgmi_bytes_per_step_per_rank", "plans", "plan"):
        if k in line:
            s[k] = line[k]
    s["detail_file"] = detail_file
    s = _finite(s)
    out = json.dumps(s, allow_nan=False, separators=(",", ":"))
    if len(out) > SUMMARY_MAX_BYTES:            # never print an unparseably long line: drop the optional blocks, largest first
        for k in ("others_ms_per_step", "stages_ms", "sustained", "eval", "default_optimizer"):
            s.pop(k, None)
            out = json.dumps(s, allow_nan=False, separators=(",", ":"))
            if len(out) <= SUMMARY_MAX_BYTES:
                break
    return out


def emit(line):
    """full result -> bench_detail.json (repo root, and gpurun_out/ when it exists); the summary -> the ONE stdout line"""
    detail = json.dumps(_finite(line), allow_nan=False, indent=1)
    for d in (ROOT, os.path.join(ROOT, "gpurun_out")):
        if os.path.isdir(d):
            try:
                with open(os.path.join(d, DETAIL_FILE), "w") as f:
                    f.write(detail + "\n")
            except OSError:
                pass
    sys.stdout.flush()
    sys.stderr.flush()
    print(summary_line(line), flush=True)


def spawn_ranks(n, argv):
    """`bench.py --gpus N` started as a plain process: start the N ranks as CHILD processes (torch.distributed.run)
    BEFORE anything here touches the GPU, pass their output through and exit with their code."""
    port = 29500 + (os.getpid() % 2000)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + argv
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3000, help="timed steps (default: > 1 s of C3 steps)")
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--workload", default="C3", choices=sorted(WORKLOADS))
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--sharding", default="both", choices=["both", "k", "batch"],
                    help="multi-GPU training plan: k = column slabs + all-reduce of partial scores; batch = batch rows split, "
                         "sparse gradient-row exchange to the owning rank, summed rows all-gathered (emgraph_amd/parallel.py); "
                         "both (default) = each is timed, the line carries both and `value` is the better one")
    ap.add_argument("--eval-triples", type=int, default=4096)
    ap.add_argument("--sustained-seconds", type=float, default=1.2, help="length of the extra sustained window (0 = skip)")
    ap.add_argument("--cpu-seconds", type=float, default=10.0, help="CPU work timed for cpu_baseline")
    ap.add_argument("--cpu-batches", type=int, default=4)
    ap.add_argument("--no-eval", action="store_true")
    ap.add_argument("--no-others", action="store_true", help="skip the secondary workloads (C3z, C3b, C3p, C1, C2, C5)")
    ap.add_argument("--quick", action="store_true", help="--no-others + no sweeps + no sustained window")
    ap.add_argument("--no-fused", action="store_true", help="A/B: separate forward / loss / backward kernels")
    ap.add_argument("--no-inplace", action="store_true", help="A/B: every gradient row through the contribution buffer")
    ap.add_argument("--no-pipeline", action="store_true", help="A/B: batch preparation on the compute stream")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-ceilings", action="store_true", help="skip tools/hbm_ceiling (the box's measured HBM ceilings)")
    ap.add_argument("--full", action="store_true",
                    help="beside the headline: HBM ceilings, sustained window, per-stage times + roofline, evaluation (C4), CPU baseline, "
                         "secondary workloads (the --no-* / --quick / --sustained-seconds / --cpu-* options trim this part)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what they computed to DIR/<name>.npy (see dump_outputs)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.quick:
        args.no_others, args.sustained_seconds = True, 0.0

    world_env = int(os.environ.get("WORLD_SIZE", "0") or 0)
    if args.gpus > 1 and world_env == 0:
        sys.exit(spawn_ranks(args.gpus, sys.argv[1:]))          # nothing has touched the GPU in this process
    if world_env and world_env != args.gpus:
        sys.exit("bench.py: --gpus %d but WORLD_SIZE=%d" % (args.gpus, world_env))

    import torch
    rank = int(os.environ.get("RANK", "0"))
    world = max(1, world_env)
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # EMG_BENCH_ONE_DEVICE: smoke-testing the N>1 code path on a 1-GPU box (all ranks on cuda:0, gloo)
    torch.cuda.set_device(0 if os.environ.get("EMG_BENCH_ONE_DEVICE") else local)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo" if os.environ.get("EMG_BENCH_ONE_DEVICE") else "nccl")

    ceilings = hbm_ceilings() if (args.full and rank == 0 and not args.no_ceilings) else None   # (a child process; also brings the clocks up)

    def run_plan(sharding, timed=True):
        """W warm-up steps + EXACTLY K timed steps (barrier + synchronize on both sides, max over ranks) of one multi-GPU plan"""
        rr = StepRunner(args.workload, args, rank, world, sharding=sharding, batch=args.batch)
        if not timed:
            rr.run(args.warmup)
            return rr, None, None, None
        rr.run(args.warmup)
        dt_, ti_ = rr.timed(args.steps)
        hd = step_summary(rr, dt_, ti_, args.steps)
        ls = rr.tr.read_loss()
        assert math.isfinite(ls), "loss is not finite"
        if world > 1:   # bytes each rank puts on the links per step
            if sharding == "batch":
                hd["xgmi_bytes_per_step_per_rank"] = int(rr.tr.xgmi_bytes / max(1, rr.tr.step_count))
                # rows a rank's optimizer updates per step (upper bounds from the count matrix): state replicated (what ran) against
                # state sharded by owner (Trainer(shard_state=True): SGD / momentum / Adagrad; same bits, same bytes on the links)
                hd["optimizer_rows_per_step_per_rank"] = {
                    "replicated_state": int(rr.tr.opt_rows_replicated_form / max(1, rr.tr.step_count)),
                    "owner_sharded_state": int(rr.tr.opt_rows_owner_form / max(1, rr.tr.step_count))}
            else:       # ring all-reduce of the (1 + eta) * B_global partial scores: 2 (N - 1) / N of the buffer out, as much in
                hd["xgmi_bytes_per_step_per_rank"] = int(2 * (world - 1) / world * 4 * (1 + rr.eta) * rr.B)
        return rr, hd, ls, (dt_, ti_)

    def finish(line):
        """rank 0 prints the line; every rank leaves the process group"""
        if rank == 0:
            emit(line)
        if world > 1:
            import torch.distributed as dist
            dist.barrier()
            dist.destroy_process_group()

    # N > 1: BOTH training plans are timed (K steps each) and the line carries both; `value` is the better one — so a scaling run
    # records north_star's split (batch rows over the ranks, RCCL exchange of gradient rows) whatever wins
    plan_names = [None] if world == 1 else (["k", "batch"] if args.sharding == "both" else [args.sharding])
    plans = {}
    r = None
    for pn in plan_names:
        if r is not None:
            r.close()
        r, hd, ls, tm = run_plan(pn)
        plans[pn] = {"head": hd, "loss": ls, "tm": tm}
    best = max(plan_names, key=lambda n: plans[n]["head"]["value"])
    if best != plan_names[-1]:
        # the stage / evaluation sections below run on the better plan's runner: it is created AND TIMED again (W + K steps), and
        # the headline is THAT timing — `value`, `stages` and `sustained` then describe one instance (the first pass stays in `plans`)
        r.close()
        first = plans[best]["head"]
        r, hd, ls, tm = run_plan(best)
        hd["first_pass_value"] = first["value"]
        plans[best] = {"head": hd, "loss": ls, "tm": tm}
    head, loss, (dt, t_issue) = plans[best]["head"], plans[best]["loss"], plans[best]["tm"]
    if args.dump_outputs:   # before anything else runs a step on r
        dump_outputs(r, loss, args.dump_outputs, write=(rank == 0))
    w = r.w
    line = {
        "metric": "positive+negative triples scored/sec at k=200, eta=20; filtered ranks/sec",
        "value": head["value"], "unit": "triples scored/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": head["ms_per_step"], "host_issue_ms_per_step": head["host_issue_ms_per_step"],
        "timed_seconds": head["seconds"], "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": args.workload + ": " + w["desc"],
                   "step": (("graph replay (emg_plan_run): fused score+loss+grad (+in-place singleton update) | descriptor-driven apply of both "
                             "tables; the next batches' corrupt+group stages ride at the front of the two launches" if getattr(r.tr, "graph", False) else
                             "one emg_plan_step call: corrupt+group (counting sort, 2 batches ahead, side streams) | fused score+loss+grad "
                             "(+in-place singleton SGD) | descriptor-driven apply (entities + relations, one launch)") if r.tr.plan is not None else
                            "host-driven: corrupt+group | scores | collective | loss | gradients | apply"),
                   "B_per_gpu": r.B0, "global_batch": r.B, "eta": r.eta, "k_int": r.k_full,
                   "k_int_per_gpu": r.k_local, "n_ent": w["n_ent"], "n_rel": w["n_rel"], "resident_batches": r.nb,
                   "parallelism": ("single" if world == 1 else
                                   ("k-sharded x%d: all-reduce of partial scores only" % world if r.sharding == "k" else
                                    "batch-sharded x%d: sparse gradient rows to owners, updated rows all-gathered" % world))},
        "loss_sum": loss,
    }
    if world > 1:
        line["xgmi_bytes_per_step_per_rank"] = head["xgmi_bytes_per_step_per_rank"]
        line["plans"] = {n: dict(_pick(plans[n]["head"], "value", "ms_per_step", "xgmi_bytes_per_step_per_rank", "optimizer_rows_per_step_per_rank"),
                                 loss_sum=plans[n]["loss"])
                         for n in plan_names}
        line["plan"] = best
    if world > 1 and r.sharding == "batch":
        # what the two forms of the gradient exchange put on the links per step and rank (uniform destinations; the sums' all-gather
        # is the same for both): FULL ROWS (implemented: every gradient row travels to the owner of its destination) against the
        # FACTORED form of the bilinear models (not implemented: a negative's row is g * q, so a group would send its subject /
        # object / relation rows to their owners, its two query rows to every owner that holds one of its negatives — all of
        # them at eta = 20 — and 12 bytes per negative)
        row, W_, Bl_, eta_ = 4 * r.k_full, world, r.B0, r.eta
        away = (W_ - 1) / W_
        owners_hit = W_ * (1 - (1 - 1 / W_) ** eta_)          # owners that hold at least one of a group's negatives
        line["exchange_bytes_model_per_step_per_rank"] = {
            "full_rows_out": int(Bl_ * ((2 + eta_) * away * (row + 8) + away * (row + 8))),
            "factored_out": int(Bl_ * (3 * away * (row + 8) + 2 * max(0.0, owners_hit - 1) * row + eta_ * away * 12)),
            "note": "measured: xgmi_bytes_per_step_per_rank (full rows out + the padded all-gather of the summed rows in)"}
    if not args.full:   # a plain run: the headline only
        r.close()
        finish(line)
        return
    if args.sustained_seconds > 0:
        n = max(args.steps, int(args.sustained_seconds / (dt / args.steps)) + 1)
        dts, tis = r.timed(n)
        line["sustained"] = step_summary(r, dts, tis, n)
    stages = r.stages()
    line["stages"] = stages
    byte_stages = [s for s in stages if isinstance(stages[s], dict) and stages[s].get("alg_bytes")]
    if byte_stages:
        dom = max(byte_stages, key=lambda s: stages[s]["ms"])
        ach = stages[dom]["GBps"]
        traffic, src = pmc_traffic(dom, args.workload, r.B, world, args)
        line["roofline"] = {"kernel": dom, "bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                            "frac": round(ach / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_source": src,
                            "alg_bytes_per_launch": stages[dom]["alg_bytes"], "avg_launch_ms": stages[dom]["ms"],
                            "avg_launch_ms_source": "HIP events around the launch on its stream, 16 instrumented steps of this run",
                            "copy_rate_torch": round(copy_rate(torch), 1)}
        if ceilings:   # this box's measured ceilings for the kernel's access mix (tools/hbm_ceiling.hip)
            line["roofline"]["ceilings_GBps"] = {k: ceilings[k] for k in ("copy4_wg16384_GBps", "copy4_nt_GBps", "read4_GBps", "write4_GBps",
                                                                          "gather_rows_u4_GBps", "rmw_rows_u4_GBps", "mix23_GBps", "mix23_nt_GBps") if k in ceilings}
            if dom == "fused" and "mix23_nt_ms" in ceilings:
                line["roofline"]["mix_ceiling"] = {"what": "the fused kernel's own access mix as a bare microkernel (23 random 1600-B rows read per "
                                                   "group, 16 written back in place, 5 streamed out non-temporally), same byte count",
                                                   "ms": ceilings["mix23_nt_ms"], "frac_of_mix_ceiling": round(ceilings["mix23_nt_ms"] / stages[dom]["ms"], 4)}
        prof = profiled_avg_us("train_fused_riders_kernel<3, 4, 1, 64, 1" if dom == "fused" else "apply_segments_kernel")
        if prof and args.workload == "C3":
            line["roofline"]["profiled"] = dict(prof, frac=round(stages[dom]["alg_bytes"] / (prof["avg_us"] * 1e-6) / 1e9 / HBM_PEAK_GBS, 4),
                                                note="rocprofv3 --kernel-trace --stats of `bench.py --no-others --no-eval` (this workload only), committed")
    if not args.no_eval:
        line["eval"] = run_eval(r, args)                           # every rank takes part (range-sharded candidates)
    cpu = cpu_baseline(r, args) if (rank == 0 and world == 1 and not args.no_cpu) else None
    r.close()
    def run_other(name):
        ro = StepRunner(name, args, rank, world)
        ro.run(20)
        n = 300 if name not in ("C3b", "C3a", "C3d") else 100
        d, ti = ro.timed(n)
        o = step_summary(ro, d, ti, n)
        o["workload"] = WORKLOADS[name]["desc"]
        o["stages"] = ro.stages()
        if name == "C3p":
            o["score_kernel_alone"] = score_kernel_alone(ro)
        ro.close()
        return o

    def default_optimizer_block(o):
        """C3 with the reference's DEFAULT optimizer (Keras Adam, constants.py:55) as a headline block of its own: value, step time and
        the roofline of its longest byte-moving stage (bytes incl. the optimizer state rows)"""
        st = o["stages"]
        bs = [k for k in st if isinstance(st[k], dict) and st[k].get("alg_bytes")]
        dom = max(bs, key=lambda k: st[k]["ms"])
        tot = sum(st[k]["alg_bytes"] for k in bs)
        return {"workload": "C3a: " + WORKLOADS["C3a"]["desc"], "value": o["value"], "unit": o["unit"], "ms_per_step": o["ms_per_step"],
                "steps": o["steps"], "host_issue_ms_per_step": o["host_issue_ms_per_step"],
                "stages_ms": {k: st[k]["ms"] for k in st if isinstance(st[k], dict) and "ms" in st[k]},
                "roofline": {"kernel": dom, "bound": "hbm", "achieved": st[dom]["GBps"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
                             "frac": round(st[dom]["GBps"] / HBM_PEAK_GBS, 4), "alg_bytes_per_launch": st[dom]["alg_bytes"],
                             "avg_launch_ms": st[dom]["ms"]},
                "step_alg_bytes": tot, "step_GBps": round(tot / (o["ms_per_step"] * 1e-3) / 1e9, 1),
                "note": "the headline `value` above is C3 as the REFERENCE can run it: above 5e5 entities EmbeddingModel.py:1266-1274 refuses "
                        "every optimizer but SGD.  This block is the same workload with the reference's default optimizer (Adam), which this "
                        "framework does run at that size: singleton negatives replayed + updated inside the scoring kernel, deferred dense pass"}

    if not args.no_others and world == 1 and args.workload == "C3":
        others = {}
        for name in ("C3z", "C3b", "C3p", "C3m", "C3s", "C3r", "C3a", "C3d", "C3g", "C1", "C2", "C5"):
            others[name] = run_other(name)
        line["others"] = others
        line["default_optimizer"] = default_optimizer_block(others["C3a"])
    if cpu is not None:
        line["cpu_baseline"] = cpu
    finish(line)


if __name__ == "__main__":
    main()
