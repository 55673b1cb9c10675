"""Device-resident training engine: what EmbeddingModel.fit's inner loop (EmbeddingModel.py:1388-1440)
needs per batch, restructured for one MI355X:

    corruption codes (Philox, on device)  ->  fused gather+score of positives and negatives
    ->  loss + dL/dscore  ->  fused backward (gradient rows, no atomics)
    ->  deterministic sort + row-sparse optimizer apply (entities, relations)

All buffers (tables, optimizer state, the whole mapped training set, per-batch scratch) are allocated
once as torch tensors and stay in HBM; a batch is a pointer offset into the resident training set
(the reference re-feeds numpy slices through tf.data each batch, EmbeddingModel.py:1044-1111,1329-1337).
No host synchronisation happens inside an epoch: the loss accumulates in a device double that the
caller reads once per epoch (the reference's per-batch `.numpy()` NaN check, :1421-1427, becomes a
per-epoch check).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib as L
from . import _switches
from . import device as D
from . import parallel

DEFAULT_LR = 0.0005            # training/_optimizer_constants.py:9
DEFAULT_MOMENTUM = 0.9         # :11
DEFAULT_DECAY_CYCLE = 0
DEFAULT_DECAY_CYCLE_MULTIPLE = 1
DEFAULT_LR_DECAY_FACTOR = 2
DEFAULT_END_LR = 1e-8
DEFAULT_SINE = False
ADAM_BETA1, ADAM_BETA2, KERAS_EPS = 0.9, 0.999, 1e-7   # tf.optimizers defaults (TF 2.2)
ADAGRAD_INIT_ACC = 0.1


def sgd_learning_rate(params, batches_count, epoch, batch):
    """Learning rate of plain SGD for (epoch, batch), both 1-based: a pure function of the optimizer parameters.

    Semantics of the reference's schedule (training/sgd.py:127-185; its TF2 port never calls it, SURVEY A-4),
    values pinned by tests/emgraph/models/test_optimizers.py:21,41-43,72-79:
      * neither 'decay_cycle' nor 'cosine_decay': constant 'lr';
      * 'cosine_decay': warm restarts.  Cycle i (i = 0, 1, ...) lasts decay_cycle * expand_factor**i epochs and
        anneals from lr / decay_lr_rate**i down to 'end_lr' along half a cosine, batch by batch;
      * fixed decay ('decay_cycle' > 0): the rate is divided by 'decay_lr_rate' at the first batch of epoch
        b_1 = decay_cycle + 1, b_(j+1) = decay_cycle + (b_j - 1) * expand_factor + 1, never below 'end_lr'
        (once 'end_lr' is reached the schedule stops)."""
    lr0 = params.get("lr", DEFAULT_LR)
    cycle = params.get("decay_cycle", DEFAULT_DECAY_CYCLE)
    end_lr = params.get("end_lr", DEFAULT_END_LR)
    expand = params.get("expand_factor", DEFAULT_DECAY_CYCLE_MULTIPLE)
    shrink = params.get("decay_lr_rate", DEFAULT_LR_DECAY_FACTOR)
    if cycle <= 0:
        return lr0
    if params.get("cosine_decay", DEFAULT_SINE):
        first, length, top = 0, cycle, lr0          # the cycle holding `epoch` covers epochs (first, first + length]
        while epoch > first + length:
            first, length, top = first + length, length * expand, top / shrink
        done = ((epoch - 1 - first) * batches_count + (batch - 1)) / (length * batches_count)
        return max(end_lr, end_lr + (top - end_lr) * 0.5 * (1 + math.cos(math.pi * done)))
    lr, boundary = lr0, cycle + 1
    while boundary <= epoch and lr > end_lr:
        lr, boundary = max(end_lr, lr / shrink), cycle + (boundary - 1) * expand + 1
    return lr


DEFAULT_STOP_EPOCH = 251       # EmbeddingModel.py:694-696
DEFAULT_STRUCTURAL_WT = 0.001  # :701-703
FOCUSE_SIZE_MESSAGE = ("Each triple must have a numeric value (the size of the training set does not match the size"
                       "of the focusE_numeric_edge_values argument.")   # :1174-1177


def focuse_fill_and_mean(values, seed=0):
    """Unknown (NaN) edge values replaced by uniform [0, 1) draws, column by column (EmbeddingModel.py:1099-1106), from a
    ``RandomState`` derived from ``seed`` — once, where the reference redraws nothing either (it writes through a view into the
    stored array) — then the mean over the columns (:1108, :716): float32 [n].  ``values`` [n] or [n, c] is not modified."""
    v = np.array(values, dtype=np.float64, copy=True)
    v = v.reshape(v.shape[0], -1)
    rs = np.random.RandomState((int(seed) * 2654435761 + 0xF0C5) & 0xFFFFFFFF)
    for col in range(v.shape[1]):
        unknown = np.isnan(v[:, col])
        v[unknown, col] = rs.uniform(size=int(unknown.sum()))
    return v.mean(axis=1).astype(np.float32) if v.shape[0] else np.zeros(0, np.float32)


def focuse_edge_weights(relations, values, normalize=True, seed=0):
    """The FocusE weight w_i of every training triple, float32 [n]: what the reference's ``fit()`` makes of
    ``focusE_numeric_edge_values`` on the host (no GPU work).

    ``relations`` [n]: the triples' relation column (labels or ids); ``values`` [n] or [n, c], NaN = unknown.  Per relation and
    column, over the known values (EmbeddingModel.py:1181-1228): min == max -> 1.0; otherwise min-max normalised to [0, 1] if
    ``normalize`` (``normalize_numeric_values``, default true) or min < 0 or max > 1; a column of a relation that is all NaN
    stays as it is.  Then ``focuse_fill_and_mean``.  The caller's array is not modified.  A length mismatch raises the
    reference's assertion (:1174-1177)."""
    relations = np.asarray(relations).reshape(-1)
    v = np.array(values, dtype=np.float64, copy=True)
    assert v.shape[0] == relations.shape[0], FOCUSE_SIZE_MESSAGE
    v = v.reshape(v.shape[0], -1)
    for reln in np.unique(relations):
        rows = relations == reln
        for col in range(v.shape[1]):
            x = v[rows, col]
            known = ~np.isnan(x)
            if not known.any():
                continue                       # all the weights are NaN
            lo, hi = x[known].min(), x[known].max()
            if lo == hi:
                v[rows, col] = 1.0
            elif normalize or lo < 0 or hi > 1:
                v[rows, col] = (x - lo) / (hi - lo)
    return focuse_fill_and_mean(v, seed)


def focuse_structure_weight(epoch, stop_epoch=DEFAULT_STOP_EPOCH, structural_wt=DEFAULT_STRUCTURAL_WT):
    """Structure weight of the 1-based ``epoch`` (EmbeddingModel.py:692-714): ``stop_epoch`` == 0: the fixed ``structural_wt``
    in [0, 1]; otherwise a linear decay from 1 that reaches its floor 0.001 at ``stop_epoch``.  (The epoch is the training
    loop's — the semantics the reference's commented-out feed_dict intended; its TF2 port pins epoch = 0.)"""
    assert stop_epoch >= 0, "Invalid value for stop_epoch"
    if stop_epoch == 0:
        assert structural_wt <= 1 and structural_wt >= 0, "Invalid structure_weight passed to model params!"
        return float(structural_wt)
    return max(1.0 - epoch / stop_epoch, 0.001)


def _padded_ld(k_int):
    """row stride: multiple of 4 floats so every row is 16-byte aligned for dwordx4 loads"""
    return ((k_int + 3) // 4) * 4


def alloc_table(rows, k_int, device, init=None, fill=None):
    ld = _padded_ld(k_int)
    buf = torch.zeros((rows, ld), dtype=torch.float32, device=device)
    view = buf[:, :k_int]
    if init is not None:   # a host array, or a device tensor (tables initialised on the device)
        view.copy_(init if torch.is_tensor(init) else torch.from_numpy(np.ascontiguousarray(init, dtype=np.float32)))
    elif fill is not None:
        view.fill_(fill)
    return view  # 2-D view with stride(0) = ld


# batches prepared ahead of the one computing (= side streams = extra batch slots); see Trainer.step.
# Two, not more: main + apply_rel stream + 2 side streams = 4 = the HIP runtime's hardware queues per device;
# a fifth stream is multiplexed onto them and the step got SLOWER (measured 0.47 -> 0.67 ms at 3, 0.73 at 4).
LOOKAHEAD = 2
LOSS_SLOTS = 64             # doubles the fused kernel spreads the batch loss over
GRAPH_MAX_ROWS = 200000     # entity contribution rows per batch up to which steps run as graph replays
AUX_MIN_ROWS = 100000       # entity contribution rows per batch above which the host-driven step gives apply_rel its own stream


class Trainer:
    """One model's device state + the per-batch step."""

    def __init__(self, model_id, k_int, scale, ent_init, rel_init, eta, loss="nll", loss_params=None,
                 optimizer="adam", optimizer_params=None, corrupt_sides=("s,o",), batches_count=1, seed=0,
                 regularizer=None, regularizer_params=None, normalize_ent_emb=False, device="cuda", fused=True,
                 inplace=True, pipeline=True, sharded=False, deferred_dense=None, shard_state=False, link="linear",
                 focuse_params=None, negative_sampler=None, shared_negatives=None):
        """``sharded=True`` / ``"k"``: ent_init / rel_init are this rank's COLUMN slabs (emgraph_amd.parallel.shard_columns)
        and k_int is the local width; every step all-reduces the partial scores.
        ``sharded="batch"``: full tables on every rank; each rank scores its rows of the global batch, gradient rows
        travel to the owner of their destination, which applies them and all-gathers the updated rows (parallel.py).
        ``shard_state=True`` (with ``sharded="batch"``; SGD / momentum / Adagrad without regulariser): the optimizer state is
        sharded by OWNER — each rank holds the state rows of its own id range only, applies the optimizer to the summed gradients of
        ITS rows and all-gathers the UPDATED rows (the same bytes as the summed gradients), which every replica copies into its
        table: 1/N of the state and of the update arithmetic, same bits.  Keras Adam cannot take this form (every row moves every
        step: the replicas would need the whole table back), nor can a folded LP regulariser.
        ``deferred_dense`` (one GPU, Adam and / or an LP regulariser; default: tables of >= 256 MB, or env EMG_ADAM_DEFERRED=0/1):
        the dense pass (Keras Adam's decay, the regulariser's gradient) is replayed only for the rows a batch reads and
        updates (emg_deferred_catchup) instead of passing over the whole table every step — same bits; ``materialize()``
        brings every row up to date before the tables are read.
        ``link``: the score non-linearity ('linear' | 'tanh' | 'sigmoid' | 'softplus', EmbeddingModel.py:679-690).
        ``focuse_params``: {'stop_epoch', 'structural_wt'} of the structure-weight schedule, read once edge weights are set
        (``set_training_set(..., edge_w=...)``).  One GPU only.
        ``negative_sampler``: {'keep_thr': uint32 [n_rel] or None, 'known_keys': int64 ascending distinct keys or None,
        'retries': int, 'type_constraints': TypeConstraints or None} (emgraph_amd.negative_sampling) — Bernoulli side choice,
        known-triple filtering and / or typed pools of the negatives.
        One GPU only; the run's steps then go through ``emg_plan_step`` (no graph replays).
        ``shared_negatives`` = C (1 <= C <= 256; DESIGN.md A-26, 4.1 "Shared negatives"): the batch is cut into chunks of C consecutive
        rows, a chunk shares ONE draw per (side, j) and every positive of it is scored against all of them — the ordinary step
        with codes[m * B + i] = chunk_codes[m * G + i // C].  One GPU, no negative sampler; host-driven steps (no plan, no graph
        replays, no in-place or factored forms, no look-ahead, the dense pass never deferred).
        ``corrupt_sides`` may hold ``'p'``, at most once (DESIGN.md A-28, 4.1 "Relation negatives"): eta draws per positive replace its
        RELATION by one of the other n_rel - 1.  Slot order: the entity sides in the order given, then 'p'.  One GPU, no negative
        sampler, no shared negatives; host-driven steps like the shared form's.
        ``regularizer`` = ``'LP'`` (the reference's: the full tables, folded into the optimizer step) or ``'batch_LP'`` / ``'N3'``
        (DESIGN.md A-29, 4.1 "Batch regulariser"): the Lp penalty — on the complex modulus for rows [re | im] unless
        ``regularizer_params['modulus']`` is false — of the rows the batch's POSITIVES look up, once per occurrence, summed over the
        batch and added to the loss ``read_loss`` reports; ``'N3'`` = ``'batch_LP'`` with p = 3 on the modulus.  One GPU, no negative
        sampler, no shared or relation negatives; host-driven steps like the relation-negatives form's."""
        from . import negative_sampling
        corrupt_sides = negative_sampling.canonical_sides(corrupt_sides)
        self.relneg = negative_sampling.RELATION_SIDE in corrupt_sides
        if self.relneg:
            if sharded:
                raise NotImplementedError("corrupt_sides with 'p' (relation negatives) is not available with sharded (multi-GPU) training")
            if shared_negatives is not None:
                raise NotImplementedError("corrupt_sides with 'p' (relation negatives) is not available with shared_negatives")
            if negative_sampler is not None:
                raise NotImplementedError("corrupt_sides with 'p' (relation negatives) is not available with a negative sampler "
                                          "(Bernoulli side choice, filtered or typed negatives)")
            if model_id == L.TRANSE_P and np.isinf(scale):
                raise NotImplementedError("corrupt_sides with 'p' (relation negatives) is not available with TransE of norm inf")
            if rel_init.shape[0] < 2:
                raise ValueError("corrupt_sides with 'p' (relation negatives) needs at least two relations, the table has "
                                 "{}".format(rel_init.shape[0]))
        if link not in L.LINK_IDS:
            raise ValueError("Invalid non-linearity")
        if sharded and link != "linear":
            raise NotImplementedError("a non-linear score link is not available with sharded (multi-GPU) training")
        if sharded and negative_sampler is not None:
            raise NotImplementedError("Bernoulli side sampling and filtered negatives are not available with sharded (multi-GPU) training")
        if model_id == L.SIMPLE and sharded:   # (before the device is asked for)
            raise NotImplementedError("SimplE trains on one GPU: sharding {!r} is not available".format(sharded))
        if model_id == L.SIMPLE and shared_negatives is not None:
            raise NotImplementedError("SimplE: shared_negatives is not available (the shared-negatives kernels have no SimplE form)")
        self.shared = None
        if shared_negatives is not None:
            if isinstance(shared_negatives, bool) or not isinstance(shared_negatives, (int, np.integer)) \
                    or not 1 <= shared_negatives <= L.SHARED_NEGATIVES_MAX:
                raise ValueError("shared_negatives must be an int in [1, {}], got {!r}".format(L.SHARED_NEGATIVES_MAX, shared_negatives))
            if sharded or negative_sampler is not None:
                raise NotImplementedError("shared_negatives is not available with sharded (multi-GPU) training or a negative sampler")
            self.shared = int(shared_negatives)
            fused = inplace = pipeline = False
            deferred_dense = False
        if self.relneg:
            fused = inplace = pipeline = False
            deferred_dense = False
        # 'batch_LP' / 'N3' (DESIGN.md A-29, 4.1 "Batch regulariser"): the penalty of the rows the batch's positives look up, its
        # gradient rows appended behind the step's own.  Not the folded full-table LP: self.reg stays None.
        self.batchreg = None
        if regularizer in negative_sampling.BATCH_REGULARIZERS:
            self.batchreg = negative_sampling.batch_regularizer_params(
                regularizer, regularizer_params, pair_rows=model_id in (L.COMPLEX, L.HOLE, L.ROTATE), phase_relations=model_id == L.ROTATE)
            if sharded:
                raise NotImplementedError("a batch regulariser ('batch_LP' / 'N3') is not available with sharded (multi-GPU) training")
            if shared_negatives is not None:
                raise NotImplementedError("a batch regulariser ('batch_LP' / 'N3') is not available with shared_negatives")
            if negative_sampler is not None:
                raise NotImplementedError("a batch regulariser ('batch_LP' / 'N3') is not available with a negative sampler "
                                          "(Bernoulli side choice, filtered or typed negatives)")
            if self.relneg:
                raise NotImplementedError("a batch regulariser ('batch_LP' / 'N3') is not available with 'p' among the corruption "
                                          "sides (relation negatives)")
            regularizer = None
            fused = inplace = pipeline = False
            deferred_dense = False
        D.require_gpu()
        self.link_id = L.LINK_IDS[link]
        fp = focuse_params or {}
        self.stop_epoch = fp.get("stop_epoch", DEFAULT_STOP_EPOCH)
        self.structural_wt = fp.get("structural_wt", DEFAULT_STRUCTURAL_WT)
        self.edge_w = None          # device float32 [n_triples]: FocusE weight of every resident triple
        self.link_fac = None        # unfused step: weight * phi'(score) of the batch
        self.device = torch.device(device)
        self.model_id, self.k_int, self.scale, self.eta = model_id, int(k_int), float(scale), int(eta)
        self.loss_id = L.LOSS_IDS[loss]
        lp = loss_params or {}
        default_margin = 3.0 if loss == "self_adversarial" else 1.0   # losses/_loss_constants.py:8-12
        self.margin = float(lp.get("margin", default_margin))
        self.alpha = float(lp.get("alpha", 0.5))
        self.sides = [L.SIDE_IDS[s] for s in corrupt_sides]
        self.n_sides = len(self.sides)            # ('p' counts: a block of eta slots behind the entity sides')
        self.eta_total = self.eta * self.n_sides
        self.seed = int(seed)
        self.batches_count = int(batches_count)
        self.normalize = bool(normalize_ent_emb)

        self.ent = alloc_table(ent_init.shape[0], k_int, self.device, init=ent_init)
        self.rel = alloc_table(rel_init.shape[0], k_int, self.device, init=rel_init)
        self.n_ent, self.n_rel = ent_init.shape[0], rel_init.shape[0]

        op = optimizer_params or {}
        self.opt_name = optimizer
        self.opt_id = L.OPT_IDS[optimizer]
        self.lr = float(op.get("lr", DEFAULT_LR))
        self.momentum = float(op.get("momentum", DEFAULT_MOMENTUM))
        self.sgd_params = dict(op) if optimizer == "sgd" else None
        self.state_ent = [None, None]
        self.state_rel = [None, None]
        if optimizer == "momentum":
            self.state_ent[0] = alloc_table(self.n_ent, k_int, self.device)
            self.state_rel[0] = alloc_table(self.n_rel, k_int, self.device)
        elif optimizer == "adagrad":
            self.state_ent[0] = alloc_table(self.n_ent, k_int, self.device, fill=ADAGRAD_INIT_ACC)
            self.state_rel[0] = alloc_table(self.n_rel, k_int, self.device, fill=ADAGRAD_INIT_ACC)
        elif optimizer in ("adam", "adam_lazy"):
            for st, n in ((self.state_ent, self.n_ent), (self.state_rel, self.n_rel)):
                st[0] = alloc_table(n, k_int, self.device)
                st[1] = alloc_table(n, k_int, self.device)
        # the negative sampler's device arrays (bound while the plan is created: emg_plan_create keeps the binding for its run)
        self.sampler = None
        self.corruption_rows = 0    # corruption rows of the steps taken, counted on the host: the 'rows' reported with no sampler
        if negative_sampler is not None:
            thr, keys = negative_sampler.get("keep_thr"), negative_sampler.get("known_keys")
            up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(self.device)  # noqa: E731
            self.sampler = {
                "keep_thr": up(np.asarray(thr, dtype=np.uint32), np.int32) if thr is not None else None,
                "known_keys": up(np.asarray(keys, dtype=np.int64), np.int64) if keys is not None and len(keys) else None,
                "retries": int(negative_sampler.get("retries", 4)),
            }
            tc = negative_sampler.get("type_constraints")
            if tc is not None and (tc.n_ent != self.n_ent or tc.n_rel != self.n_rel):
                raise ValueError("the type constraints of the negative sampler were built for tables of another size")
            # typed negatives: the pools on the device, and a fourth counter (rows drawn from a non-empty pool)
            self.sampler["pools"] = tc.device(self.device) if tc is not None else None
            self.sampler["stats"] = torch.zeros(4 if tc is not None else 3, dtype=torch.int64, device=self.device)
        self.tag_ent = torch.zeros(self.n_ent, dtype=torch.int32, device=self.device)
        self.tag_rel = torch.zeros(self.n_rel, dtype=torch.int32, device=self.device)
        self.step_count = 0

        self.reg = None
        if regularizer is not None:
            rp = regularizer_params or {}
            lam = rp.get("lambda", 1e-5)      # regularizers/_regularizer_constants.py:8-10
            p = rp.get("p", 2)
            if not isinstance(p, (int, np.integer)):
                raise Exception("Invalid value for regularizer parameter p:{}. Supported type int, np.int32 or "
                                "np.int64".format(p))
            if np.isscalar(lam):
                lam = [lam, lam]
            elif not (isinstance(lam, list) and len(lam) == 2):
                raise ValueError("Regularizer weight must be a scalar or a list with length equal to number of "
                                 "params passes")
            self.reg = (float(lam[0]), float(lam[1]), int(p))
        # The LP penalty covers the full tables (lp.py:107-113), so its gradient is dense.  It is FOLDED into the
        # optimizer step: rows with contributions (or updated in place) add lambda*p*|w|^(p-1)*sign(w) to their summed
        # gradient, all other rows get it in one dense pass (emg_apply_grouped / untouched_rows_kernel) — no extra
        # contribution rows, one update per row per step with the gradient of the whole loss.
        self.reg_rows = False

        self.plan = None
        self.graph = False
        # the data loss: LOSS_SLOTS doubles, workgroup b of the fused kernel adds to slot b mod LOSS_SLOTS (same-address atomics of a
        # short launch queue up behind each other: include/emgraph_hip.h, emg_backward_args.loss_slots); every other producer adds to
        # slot 0; read_loss sums
        self.loss_accum = torch.zeros(LOSS_SLOTS, dtype=torch.float64, device=self.device)
        self.reg_accum = torch.zeros(1, dtype=torch.float64, device=self.device)  # LP term (column-local when sharded)
        # sum |w|^p per table, accumulated by the kernels that fold the regulariser (scaled by lambda in read_loss)
        self.lp_sum = torch.zeros(2, dtype=torch.float64, device=self.device)
        self.X = None
        self._cap = 0
        self.stage_events = None  # filled by enable_stage_timing()
        # execution plan
        #  fused   : score -> pair-local loss -> gradient in ONE kernel (pairwise / nll / absolute_margin)
        #  inplace : rows whose destination is hit once in the batch are updated from registers
        #            (plain SGD only: _choose_inplace)
        #  pipeline: codes + destination grouping of batches t+1, t+2 run on a side stream while batch t computes
        self.batch_sharded = sharded == "batch"
        self.sharded = bool(sharded) and not self.batch_sharded          # k (column) sharding
        # rows wider than 512 columns (per half for ComplEx / HolE) do not fit the register-tiled kernels: the separate
        # forward / loss / backward path handles them in column blocks (emg_score.hip::run_group_pass)
        self.wide = (self.k_int // 2 if model_id in (L.COMPLEX, L.HOLE) else self.k_int) > 512
        # TransE with an order of the norm other than 1 / 2 (EMG_TRANSE_P; `scale` carries the order): generic kernels — the separate
        # forward / loss / backward step, every gradient row through the apply.  RotatE (EMG_ROTATE) and SimplE (EMG_SIMPLE) train the same way.
        self.generic = model_id in (L.TRANSE_P, L.ROTATE, L.SIMPLE)
        if model_id == L.ROTATE and sharded:
            raise NotImplementedError("RotatE trains on one GPU: sharding {!r} is not available".format(sharded))
        if self.generic and self.sharded:
            raise ValueError("TransE with a norm other than 1 / 2 does not train on column slabs (sharding 'k'): use sharding 'batch'")
        self.fused = fused and loss in ("pairwise", "nll", "absolute_margin") and not self.sharded and not self.wide and not self.generic
        # (an LP regulariser is folded into every update: by the apply kernel, and by the in-place form of plain SGD — its
        # own instantiation (IP 3), so that the pow / sign code stays out of the forms that have no regulariser)
        n_cols = self.k_int // 2 if model_id in (L.COMPLEX, L.HOLE) else self.k_int
        self.inplace_mode = 0   # 0 off | 1 singletons in place | 2 the same through a stateful optimizer's window form (_choose_inplace)
        self.inplace = self._inplace_wanted = inplace and not self.generic and (self.reg is None or (self.opt_id == L.OPT_SGD and self.reg[2] <= 3
                                                                                and n_cols % 4 == 0))
        # default: on where the dense pass is what a step costs — an entity table of 256 MB or more (C3 with Adam: 2.6 -> 1.65
        # ms/step); small tables keep the dense pass (6-14 us at C1 / C2 / C5, inside the step graph)
        env_def = _switches.get("EMG_ADAM_DEFERRED")
        want_deferred = deferred_dense if deferred_dense is not None else \
            (env_def == "1" if env_def in ("0", "1") else self.n_ent * k_int * 4 >= (256 << 20))
        # (what has a dense pass at all: Keras Adam's decay, the LP regulariser's gradient)
        self.deferred = bool(want_deferred) and (self.opt_id == L.OPT_ADAM or self.reg is not None) and not self.sharded \
            and not self.batch_sharded and not normalize_ent_emb
        self._lr_t_hist = None          # device float32 [steps]: learning rate (Adam: lr_t) of every optimizer step (deferred pass)
        self._lr_t_filled = 0
        self._lr_host = [0.0]           # host copy (index = step)
        #  factored: bilinear models write a negative's gradient row as (one float) x (one of the group's two query
        #            rows) instead of eta full rows per group (emg_backward_args.fac_ws_ent); EMG_FACTORED=0 = A/B switch
        self.factored = (model_id not in (L.TRANSE_L1, L.TRANSE_L2, L.TRANSE_P, L.ROTATE, L.SIMPLE) and not self.batch_sharded
                         and _switches.get("EMG_FACTORED") != "0" and self.shared is None and not self.relneg
                         and self.batchreg is None)
        self.pipeline = pipeline
        if self.batch_sharded:
            # a destination's contributions come from several ranks: no rank may update a row in place, and the
            # step has collectives in the middle (single stream; the exchange is what bounds it, not the enqueue).
            # Optimizer state is REPLICATED: the owner of a destination only SUMS its rows (in global slot order), the sums
            # are all-gathered and every replica applies the optimizer to them — touched rows from the sums, all others
            # through the dense pass — so Keras' dense-equivalent Adam and the folded LP regulariser work as on one GPU.
            self.inplace = self.pipeline = pipeline = False
            self.xgmi_bytes = 0          # bytes this rank sent + received over the interconnect (gradient rows + summed rows)
            self._owner_ws = {}
            # device-resident exchange (parallel.RowExchange; round 4): sizes settled in a table-independent metadata phase, the owner's
            # order by a keyed counting grouping — which needs a range of at most 2^20 + 16 n rows per owner; otherwise (or with
            # EMG_GROUPING=sort) round 3's host-driven exchange (argsort / unique, a count exchange and fresh buffers every step)
            _, world = parallel.rank_world()
            self._device_exchange = (_switches.get("EMG_GROUPING") != "sort"
                                     and -(-max(self.n_ent, self.n_rel) // max(1, world)) <= (1 << 20))
            self._xchg_objs, self._gslot_cache = {}, {}
            # rows this rank's optimizer updated (upper bounds from the count matrix: no host read), and what the other form would have
            self.opt_rows = self.opt_rows_owner_form = self.opt_rows_replicated_form = 0
            self._bs_ready = {}          # batches whose metadata phase has been issued ahead: key -> prepared state
            self._bs_parity = 0
            self._bs_done = [torch.cuda.Event(), torch.cuda.Event()]   # main-stream work that last used slot / workspaces of a parity
            self._bs_ahead = self._device_exchange
            self._bs_stream = torch.cuda.Stream(device=self.device) if self._bs_ahead else None
        self.shard_state = bool(shard_state)
        if self.shard_state:
            if not self.batch_sharded or self.opt_id not in (L.OPT_SGD, L.OPT_MOMENTUM, L.OPT_ADAGRAD) or self.reg is not None:
                raise ValueError("shard_state needs sharded='batch' and SGD / momentum / Adagrad without a regulariser (Keras Adam and the "
                                 "LP regulariser move every row every step: their state cannot live at the owner alone)")
            if not self._device_exchange:
                raise ValueError("shard_state needs the device-resident exchange (owner ranges of <= 2^20 rows + 16 per slot, not EMG_GROUPING=sort)")
            rank_, world_ = parallel.rank_world()
            for st_, n_ in ((self.state_ent, self.n_ent), (self.state_rel, self.n_rel)):
                e0_, e1_ = parallel.entity_range(n_, rank_, world_)
                if st_[0] is not None:   # this rank's rows only
                    st_[0] = alloc_table(max(1, e1_ - e0_), k_int, self.device, fill=ADAGRAD_INIT_ACC if optimizer == "adagrad" else None)
        # high priority: the many small kernels must not queue behind the big ones.  TWO side streams used
        # alternately: a preparation chain is latency-bound (each small launch waits for a CU slot), so two
        # chains in flight double the rate at which prepared batches arrive
        self.lookahead = LOOKAHEAD if pipeline else 0
        self.sides_st = [torch.cuda.Stream(device=self.device, priority=-1) for _ in range(self.lookahead)]
        self._side_rr = 0
        self.aux = torch.cuda.Stream(device=self.device) if self.pipeline else None  # apply_rel under apply_ent
        self.aux_fork, self.aux_join = torch.cuda.Event(), torch.cuda.Event()
        self.slots = []

    # ---- data ----
    def set_training_set(self, X_idx, batch_size, edge_w=None):
        """Upload the whole mapped training set once; allocate per-batch scratch for ``batch_size``.  ``edge_w`` (float32 [n],
        focuse_edge_weights): the FocusE weight of every triple, uploaded beside it."""
        X_idx = np.ascontiguousarray(X_idx, dtype=np.int32)
        self.X = torch.from_numpy(X_idx).to(self.device)
        self.edge_w = None
        if edge_w is not None:
            if self.sharded or self.batch_sharded:
                raise NotImplementedError("FocusE edge weights are not available with sharded (multi-GPU) training")
            edge_w = np.ascontiguousarray(edge_w, dtype=np.float32).reshape(-1)
            assert edge_w.shape[0] == X_idx.shape[0], FOCUSE_SIZE_MESSAGE
            focuse_structure_weight(1, self.stop_epoch, self.structural_wt)   # (the range checks, before the first step)
            self.edge_w = torch.from_numpy(edge_w).to(self.device)
        if int(batch_size) <= self._cap:
            self._alloc_link_fac(self._cap)
            self._make_plan()            # the plan points at the resident training set
        self._alloc_scratch(int(batch_size))

    @property
    def linked(self):
        """a score link and / or FocusE edge weights act on the scores of this run"""
        return self.link_id != L.LINK_LINEAR or self.edge_w is not None

    def _alloc_link_fac(self, B):
        """the unfused step's weight * phi'(score) of a batch of B positives (emg_plan_config.link_fac)"""
        self.link_fac = (torch.empty(B * (1 + self.eta_total), dtype=torch.float32, device=self.device)
                         if (self.linked and not self.fused) else None)

    def _choose_inplace(self, B):
        """In-place singleton updates: the fused kernel reads a singleton's row anyway and writes it back updated — no contribution
        row, and the apply never sees 70 % of C3's slots.  Plain SGD always takes it.  A STATEFUL optimizer takes it where the
        kernel can fetch the optimizer state rows together with the table row (round 4: fused kernels, 16-byte rows of at most 64
        chunks — emg_score_kernels.hpp::ip_traits 4 / 5 / 6): round 3's form read the state at the update, a dependent round trip
        per row at one wave per SIMD, and lost to the apply everywhere (C1 Adam 0.081 / 0.078 ms per step in place / through the
        apply, C3 Adagrad 0.842 / 0.755).  Under the deferred dense pass (Adam on a large table) the singletons among the negatives
        are replayed inside the kernel as they are gathered: (w, m, v) read once and written once where catch-up + scoring + apply
        moved the row twelve times.  Results are the same bits either way (one optimizer rule, one summation order:
        tests/test_config_widths.py::test_inplace_choice_does_not_change_bits)."""
        if not self._inplace_wanted or self.batch_sharded:
            return 0
        stateful = self.opt_id != L.OPT_SGD
        n_cols = self.k_int // 2 if self.model_id in (L.COMPLEX, L.HOLE) else self.k_int
        window = self.fused and n_cols % 4 == 0 and n_cols // 4 <= 64 and _switches.get("EMG_INPLACE_STATE") != "0"
        # what CAN run in place: SGD anything; a stateful optimizer anything (window form or chunk-wise) unless its dense pass is
        # deferred — then only Adam through the window form's replay, finished by the descriptor-driven apply (rows of > 16 chunks)
        can = not (stateful and self.deferred) or (window and self.opt_id == L.OPT_ADAM and self.reg is None and self.k_int > 64)
        # modes: 1 = singletons in place (SGD; a stateful optimizer's chunk-wise form), 2 = a stateful optimizer's window form
        mode = 2 if (stateful and window) else 1
        if _switches.get("EMG_INPLACE") in ("0", "1"):      # A/B aid
            return mode if (_switches.get("EMG_INPLACE") == "1" and can) else 0
        if not stateful:
            return mode if can else 0
        # small batches (the graph-replay range) stay with the apply: its launch is latency-bound there and does not shrink with its
        # item count, so the in-place work only lengthens the scoring kernel (measured: C1 0.0778 / 0.0747, C2 0.0637 / 0.0585, C5
        # 0.1527 / 0.1319 ms per step in place / through the apply; C3 Adagrad 0.612 / 0.695, C3 Adam 0.90 / 1.15)
        return 2 if (can and window and (2 + self.eta_total) * B > GRAPH_MAX_ROWS) else 0

    def _settle_deferred(self, B):
        """decide, BEFORE the in-place form is chosen from it, whether the deferred dense pass can go on with scratch for B positives
        (it lives in the plan's step and walks the counting / bucket grouping's descriptors); if it ends after steps have run, the
        lagging rows and their state are brought up to date first"""
        if not self.deferred:
            return
        ok = not (self.sharded or self.batch_sharded or self.X is None)
        ok = ok and bool(L.load().emg_plan_deferred_ok(B, self.eta_total, self.n_ent, self.n_rel))
        if not ok:
            self.materialize()
            self.deferred = False

    def _alloc_scratch(self, B):
        if B <= self._cap:
            return
        self._settle_deferred(B)
        self.inplace_mode = self._choose_inplace(B)
        if self.inplace_mode == 2 and self.sharded:
            self.inplace_mode = 1      # (the window form is the plan's; host-driven steps keep the chunk-wise form)
        self.inplace = self.inplace_mode != 0
        torch.cuda.synchronize()
        dev, k, et = self.device, self.k_int, self.eta_total
        ldc = _padded_ld(k)
        xe = self.n_ent if self.reg_rows else 0
        xr = self.n_rel if self.reg_rows else 0
        n_ce, n_cr = (2 + et) * B + xe, B + xr
        n_codes = B * et
        if self.shared is not None:     # one gradient row and one code per (chunk, side, j) instead of per (positive, side, j)
            n_codes = -(-B // self.shared) * et
            n_ce = 2 * B + n_codes + xe
        if self.relneg:                 # the entity sides' rows, then the relation side's 2 B; relation rows: B + one per relation draw
            n_ce = (4 + et - self.eta) * B + xe
            n_cr = (1 + self.eta) * B + xr
        if self.batchreg is not None:   # the regulariser's 2 B entity rows and B relation rows, behind the step's own
            n_ce += 2 * B
            n_cr += B
        self.scores_all = torch.empty(B * (1 + et), dtype=torch.float32, device=dev)  # [pos | neg], one all-reduce
        self.g_all = torch.empty(B * (1 + et), dtype=torch.float32, device=dev)       # dL/dscore, same layout
        self.g_pos, self.g_neg = self.g_all[:B], self.g_all[B:]
        self._alloc_link_fac(B)
        # factored: subject rows | object rows | query rows (object side) | query rows (subject side)
        self.contrib_ent = torch.empty((4 * B if self.factored else n_ce, ldc), dtype=torch.float32, device=dev)[:, :k]
        self.contrib_rel = torch.empty((n_cr, ldc), dtype=torch.float32, device=dev)[:, :k]
        self.slots = []
        n_slots = 2 if (self.batch_sharded and getattr(self, "_bs_ahead", False)) else 1 + self.lookahead
        for _ in range(n_slots):  # current batch + the ones being prepared ahead
            sl = {
                "codes": torch.empty(n_codes, dtype=torch.int32, device=dev),
                "dest_ent": torch.empty(n_ce, dtype=torch.int32, device=dev),
                "dest_rel": torch.empty(n_cr, dtype=torch.int32, device=dev),
                "single": torch.empty(n_ce, dtype=torch.uint8, device=dev),
                "ws_ent": torch.empty(D.apply_workspace_bytes(n_ce, self.n_ent, k), dtype=torch.uint8, device=dev),
                "ws_rel": torch.empty(D.apply_workspace_bytes(n_cr, self.n_rel, k), dtype=torch.uint8, device=dev),
                "ready": torch.cuda.Event(), "done": torch.cuda.Event(), "key": None,
            }
            if self.reg_rows:  # LP gradient rows come FIRST ([0, n_rows)); their destinations never change
                sl["dest_ent"][:xe] = torch.arange(self.n_ent, dtype=torch.int32, device=dev)
                sl["dest_rel"][:xr] = torch.arange(self.n_rel, dtype=torch.int32, device=dev)
            self.slots.append(sl)
        self._cap = B
        self._xe, self._xr = xe, xr
        torch.cuda.synchronize()
        self._make_plan()

    # ---- the step plan in the library (emg_plan.hip): one call per batch instead of a dozen ----
    def _make_plan(self):
        import ctypes as C
        if self.plan is not None:
            L.check(L.load().emg_plan_destroy(self.plan), "emg_plan_destroy")
            self.plan = None
        if self.sharded or self.batch_sharded or self.X is None or self.shared is not None or self.relneg \
                or self.batchreg is not None:
            self.materialize()      # (no-op unless deferred steps have run)
            self.deferred = False   # (the deferred dense decay lives in the plan's step)
            return   # multi-GPU steps have a collective in the middle: driven from the host (see step / _compute)
        c = L.PlanConfig()
        c.model, c.k_int, c.scale, c.eta, c.n_sides = self.model_id, self.k_int, self.scale, self.eta, self.n_sides
        for i, sd in enumerate(self.sides):
            c.sides[i] = sd
        c.ent, c.n_ent, c.ld_ent = self.ent.data_ptr(), self.n_ent, self.ent.stride(0)
        c.rel, c.n_rel, c.ld_rel = self.rel.data_ptr(), self.n_rel, self.rel.stride(0)
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        c.ent_state0, c.ent_state1 = ptr(self.state_ent[0]), ptr(self.state_ent[1])
        c.rel_state0, c.rel_state1 = ptr(self.state_rel[0]), ptr(self.state_rel[1])
        c.tag_ent, c.tag_rel = self.tag_ent.data_ptr(), self.tag_rel.data_ptr()
        c.opt, c.loss, c.margin, c.alpha = self.opt_id, self.loss_id, self.margin, self.alpha
        c.seed, c.batches_count = self.seed & 0xFFFFFFFFFFFFFFFF, self.batches_count
        c.X, c.n_triples, c.cap_B = self.X.data_ptr(), self.X.shape[0], self._cap
        c.scores, c.g = self.scores_all.data_ptr(), self.g_all.data_ptr()
        c.contrib_ent, c.contrib_rel, c.ldc = self.contrib_ent.data_ptr(), self.contrib_rel.data_ptr(), self.contrib_ent.stride(0)
        c.loss_accum, c.lp_sum = self.loss_accum.data_ptr(), self.lp_sum.data_ptr()
        c.loss_slots = LOSS_SLOTS
        c.factored = int(self.factored)
        if self.reg is not None:
            c.lp_lambda_ent, c.lp_lambda_rel, c.lp_p = self.reg[0], self.reg[1], self.reg[2]
        c.fused, c.inplace, c.normalize = int(self.fused), int(self.inplace_mode), int(self.normalize)
        c.n_slots = len(self.slots)
        for i, sl in enumerate(self.slots):
            ps = c.slots[i]
            ps.codes, ps.dest_ent, ps.dest_rel = sl["codes"].data_ptr(), sl["dest_ent"].data_ptr(), sl["dest_rel"].data_ptr()
            ps.single = sl["single"].data_ptr()
            ps.ws_ent, ps.ws_ent_bytes = sl["ws_ent"].data_ptr(), sl["ws_ent"].numel()
            ps.ws_rel, ps.ws_rel_bytes = sl["ws_rel"].data_ptr(), sl["ws_rel"].numel()
        self._ctl_buf = torch.zeros(4096, dtype=torch.uint8, device=self.device)   # emg_step_ctl records of a graph replay
        c.ctl_buf, c.ctl_bytes = self._ctl_buf.data_ptr(), self._ctl_buf.numel()
        if self.deferred and not L.load().emg_plan_deferred_ok(self._cap, self.eta_total, self.n_ent, self.n_rel):
            # the catch-up walks the counting grouping's segment descriptors; a table far longer than a batch has gradient
            # rows (or EMG_GROUPING=sort) is grouped by the radix-sort backend: keep the dense pass there
            self.materialize()
            self.deferred = False
        if self.deferred:
            if self._lr_t_hist is None:
                self._lr_t_hist = torch.zeros(self.LR_TABLE_STEPS, dtype=torch.float32, device=self.device)
            c.lr_t_hist = self._lr_t_hist.data_ptr()
        c.link = self.link_id
        c.edge_w = self.edge_w.data_ptr() if self.edge_w is not None else None
        c.link_fac = self.link_fac.data_ptr() if self.link_fac is not None else None
        h = C.c_void_p()
        if self.sampler is not None:
            # (the binding is one per process and not re-entrant: never taken over from, or removed under, another owner)
            if D.sampler_bound():
                raise RuntimeError("a negative sampler is already bound to the library (emg_sampler_bind is not re-entrant)")
            sm = self.sampler
            pools = sm["pools"] or (None, None)
            D.sampler_bind(self.n_ent, self.n_rel, keep_thr=sm["keep_thr"], known_keys=sm["known_keys"], retries=sm["retries"],
                           stats=sm["stats"], pool_ptr=pools[0], pool_idx=pools[1])
        try:
            L.check(L.load().emg_plan_create(C.byref(c), C.byref(h)), "emg_plan_create")
        finally:
            if self.sampler is not None:
                D.sampler_unbind()      # (the plan keeps its copy; other models of the process draw as ever)
        self.plan = h
        self._plan_cfg = c   # keeps nothing alive the tensors do not, but documents what the plan points at
        # Steps as graph replays (emg_plan_run) where a step is shorter than its launches take to issue: small batches.
        # EMG_GRAPH=1 / 0 forces it on (where the plan can) / off.
        n_ce = (2 + self.eta_total) * self._cap
        env = _switches.get("EMG_GRAPH")
        self.graph = bool(L.load().emg_plan_graph_ok(self.plan)) and (env == "1" or (env != "0" and n_ce <= GRAPH_MAX_ROWS))

    def negative_sampling_stats(self):
        """{'rows', 'redrawn', 'known_left'} over the steps taken so far: corruption rows drawn, rows whose final attempt is a
        redraw, rows whose final candidate is a known triple — counted on the device by the sampler (one read here); with no
        sampler: the host's row count and zeros"""
        if self.sampler is None:
            return {"rows": int(self.corruption_rows), "redrawn": 0, "known_left": 0}
        torch.cuda.synchronize()
        r = self.sampler["stats"].cpu().numpy()
        out = {"rows": int(r[0]), "redrawn": int(r[1]), "known_left": int(r[2])}
        if self.sampler["pools"] is not None:
            out["typed_rows"] = int(r[3])
        return out

    def __del__(self):
        try:
            if getattr(self, "plan", None) is not None:
                L.load().emg_plan_destroy(self.plan)
                self.plan = None
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass

    def _plan_batch(self, out, spec):
        start, B, epoch, batch = spec[:4]
        out.start, out.B, out.epoch, out.batch = int(start), int(B), int(epoch), int(batch)
        nc = spec[4] if len(spec) > 4 else None
        el = spec[5] if len(spec) > 5 else None
        out.n_choices = int(nc) if nc is not None else 0
        out.entities_list = el.data_ptr() if el is not None else None
        out.inj_mask = out.inj_repl = None
        out.sw = focuse_structure_weight(int(epoch), self.stop_epoch, self.structural_wt) if self.edge_w is not None else 0.0
        return el

    def _plan_step(self, start, B, epoch, batch, n_choices, entities_list, inj_mask, inj_repl, prefetch):
        import ctypes as C
        self._deferred_table_check(1)
        self.step_count += 1
        lr = (sgd_learning_rate(self.sgd_params, self.batches_count, epoch, batch) if self.sgd_params is not None
              else self.lr)
        if self.deferred:
            self._fill_lr_t(self.step_count, lr)
        cur = L.PlanBatch()
        keep = [self._plan_batch(cur, (start, B, epoch, batch, n_choices, entities_list)), inj_mask, inj_repl]
        if inj_repl is not None:
            cur.inj_repl = inj_repl.data_ptr()
            cur.inj_mask = inj_mask.data_ptr() if inj_mask is not None else None
        nxt = (L.PlanBatch * 3)()
        n_next = 0
        if prefetch is not None:
            for pf in ([prefetch] if isinstance(prefetch, tuple) else list(prefetch))[:3]:
                if pf is None or pf[1] <= 0:
                    continue
                spec = tuple(pf) if len(pf) > 4 else tuple(pf[:4]) + (n_choices, entities_list)
                keep.append(self._plan_batch(nxt[n_next], spec))
                n_next += 1
        h6 = (C.c_float * 6)(*self._hyper(lr))
        L.check(L.load().emg_plan_step(self.plan, C.byref(cur), self.step_count, h6, nxt, n_next,
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)), "emg_plan_step")

    # ---- optional per-stage HIP-event timing (bench.py) ----
    def enable_stage_timing(self, max_samples=16):
        """per-stage HIP events for the next ``max_samples`` launches of each stage (creating and recording ~10
        timing events per step costs ~0.1 ms of host time: sampling keeps long runs from turning host-bound)"""
        self.stage_events = {}
        self._stage_max = int(max_samples)
        if self.plan is not None:
            L.check(L.load().emg_plan_timing(self.plan, int(max_samples)), "emg_plan_timing")

    def _timed(self, name, fn):
        if self.stage_events is None or len(self.stage_events.get(name, ())) >= self._stage_max:
            return fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st = D.active_stream()
        e0.record(st)
        r = fn()
        e1.record(st)
        self.stage_events.setdefault(name, []).append((e0, e1))
        return r

    def stage_times_ms(self):
        torch.cuda.synchronize()
        if self.plan is not None:
            import ctypes as C
            ms, cnt = (C.c_float * 9)(), (C.c_int32 * 9)()
            L.check(L.load().emg_plan_stage_ms(self.plan, ms, cnt), "emg_plan_stage_ms")
            names = ("prepare", "fused", "forward", "loss", "backward", "apply_ent", "apply_rel", "clip", "catchup")
            return {n: [float(ms[i])] for i, n in enumerate(names) if cnt[i] > 0}
        return {k: [a.elapsed_time(b) for a, b in v] for k, v in (self.stage_events or {}).items()}

    # ---- one batch ----
    def _hyper(self, lr, table=None):
        """(lr, momentum, beta1, beta2, eps, lr_t) + (lambda, p) of the folded LP regulariser for table 0 (entities)
        / 1 (relations); table=None: no regulariser folded in"""
        t = self.step_count
        lr_t = lr * math.sqrt(1.0 - ADAM_BETA2 ** t) / (1.0 - ADAM_BETA1 ** t)
        h = (lr, self.momentum, ADAM_BETA1, ADAM_BETA2, KERAS_EPS, lr_t)
        if table is None or self.reg is None:
            return h
        return h + (self.reg[table], float(self.reg[2]))

    def _prepare(self, sl, start, B, epoch, batch, n_choices, entities_list, inj_mask, inj_repl):
        """Everything about a batch that does not depend on the tables: corruption codes (Philox, draw counter
        a pure function of (epoch, batch, side) so a refit reproduces the same negatives), destination ids of
        the gradient rows, their stable grouping and the singleton flags."""
        et, eta = self.eta_total, self.eta
        pos = self.X[start:start + B]
        n_choices = self.n_ent if n_choices is None else int(n_choices)
        if self.shared is not None:
            return self._prepare_shared(sl, start, B, epoch, batch, n_choices, entities_list, inj_mask, inj_repl)
        if self.relneg:
            return self._prepare_relneg(sl, start, B, epoch, batch, n_choices, entities_list, inj_mask, inj_repl)
        if self.batchreg is not None:
            return self._prepare_batchreg(sl, start, B, epoch, batch, n_choices, entities_list, inj_mask, inj_repl)
        codes = sl["codes"][:B * et]

        def run():
            # draw counter of side sd = ((epoch-1)*batches_count + (batch-1))*n_sides + sd
            counter0 = ((epoch - 1) * self.batches_count + (batch - 1)) * self.n_sides
            xe, xr = self._xe, self._xr
            n_ce = (2 + et) * B
            D.prepare_batch(pos, eta, self.sides, n_choices, codes, sl["dest_ent"][:xe + n_ce], sl["dest_rel"][:xr + B],
                            self.n_ent, self.n_rel, sl["ws_ent"], sl["ws_rel"], entities_list=entities_list,
                            seed=self.seed, counter0=counter0, inj_mask=inj_mask, inj_repl=inj_repl, n_extra_ent=xe,
                            n_extra_rel=xr, single_flags=sl["single"][:n_ce] if self.inplace else None,
                            factored=self.factored)

        if self.pipeline:
            side = self.sides_st[self._side_rr]
            self._side_rr = (self._side_rr + 1) % len(self.sides_st)
            side.wait_event(sl["done"])  # the compute that last used this slot has finished
            if sl["key"] is not None:    # evicting a prepared-but-never-consumed slot (caller's prefetch list did
                side.wait_event(sl["ready"])  # not match its steps): its chain may still run on the other side stream
            with D.on_stream(side):
                self._timed("prepare", run)
                sl["ready"].record(side)
        else:
            self._timed("prepare", run)
        sl["key"] = (start, B, epoch, batch)

    def step(self, start, B, epoch=1, batch=1, n_choices=None, entities_list=None, inj_mask=None, inj_repl=None,
             prefetch=None):
        """Train on resident triples [start, start+B).  ``prefetch`` = (start, B, epoch, batch[, n_choices,
        entities_list]) of the NEXT batch — or a list of the next two — lets their preparation overlap this
        batch's compute.  Two ahead matters: the preparation chain (~14 small dependent launches) takes about one
        step of wall time when it shares the GPU with the big kernels, so one batch of lookahead leaves it on the
        critical path."""
        if B <= 0:
            return
        self.corruption_rows += (B if self.shared is None else -(-B // self.shared)) * self.eta_total
        if self.batch_sharded:
            return self._step_batch_sharded(start, B, epoch, batch, n_choices, entities_list, prefetch)
        self._alloc_scratch(B)
        if self.plan is not None:
            return self._plan_step(start, B, epoch, batch, n_choices, entities_list, inj_mask, inj_repl, prefetch)
        if self.sampler is not None:
            raise RuntimeError("the negative sampler lives in the step plan: call set_training_set() first")
        self.step_count += 1
        key = (start, B, epoch, batch)
        sl = next((s for s in self.slots if s["key"] == key), None)
        if sl is None:
            sl = self.slots[0] if not self.pipeline else min(self.slots, key=lambda s: s["key"] is not None)
            self._prepare(sl, start, B, epoch, batch, n_choices, entities_list, inj_mask, inj_repl)
        if self.pipeline and prefetch is not None:
            # one batch or a list of the next ones (nearest first): each goes to a free slot unless already held
            upcoming = [prefetch] if isinstance(prefetch, tuple) else list(prefetch)
            for pf in upcoming:
                if pf is None or pf[1] <= 0 or any(s["key"] == tuple(pf[:4]) for s in self.slots):
                    continue
                free = next((s for s in self.slots if s is not sl and s["key"] is None), None)
                if free is None:
                    break
                self._prepare(free, pf[0], pf[1], pf[2], pf[3], pf[4] if len(pf) > 4 else n_choices,
                              pf[5] if len(pf) > 5 else entities_list, None, None)
        main = torch.cuda.current_stream()  # looked up once per step; every call below is routed explicitly
        if self.pipeline:
            main.wait_event(sl["ready"])
        with D.on_stream(main):
            self._compute(sl, start, B, epoch, batch, main)
        if self.pipeline:
            sl["done"].record(main)
        sl["key"] = None

    def run_batches(self, specs):
        """Train on a sequence of batches: ``specs`` = [(start, B, epoch, batch[, n_choices, entities_list]), ...] (empty
        batches allowed).  Small batches run as graph replays — one library call for the whole sequence
        (emg_plan_run: two launches per 32 steps from the host); otherwise one ``step`` per batch with the next batches
        prepared ahead."""
        specs = [s for s in specs if s is not None and s[1] > 0]
        if not specs:
            return
        if not (self.plan is not None and self.graph and self.stage_events is None):
            for i, s in enumerate(specs):
                self.step(s[0], s[1], epoch=s[2], batch=s[3], n_choices=s[4] if len(s) > 4 else None,
                          entities_list=s[5] if len(s) > 5 else None, prefetch=specs[i + 1:i + 4])
            return
        import ctypes as C
        self._alloc_scratch(max(s[1] for s in specs))
        n = len(specs)
        arr = (L.PlanBatch * n)()
        hyp = (C.c_float * (6 * n))()
        keep = []
        first = self.step_count + 1
        for i, s in enumerate(specs):
            keep.append(self._plan_batch(arr[i], s))
            self.step_count += 1
            self.corruption_rows += int(s[1]) * self.eta_total
            lr = (sgd_learning_rate(self.sgd_params, self.batches_count, s[2], s[3]) if self.sgd_params is not None else self.lr)
            hyp[6 * i:6 * i + 6] = self._hyper(lr)
        L.check(L.load().emg_plan_run(self.plan, arr, n, first, hyp, C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                "emg_plan_run")

    # ---- shared negatives (DESIGN.md 4.1 "Shared negatives") ----
    def _prepare_shared(self, sl, start, B, epoch, batch, n_choices, entities_list, inj_mask, inj_repl):
        """ONE draw per (chunk, side, j): side sd's codes are emg_corrupt_codes with B := G = ceil(B / C) under the ordinary step's
        counter of that side, so C = 1 draws what the ordinary step draws"""
        if inj_mask is not None or inj_repl is not None:
            raise ValueError("injected draws are not available with shared_negatives (drive the ordinary step with "
                             "device.expand_shared_codes instead)")
        G, eta = -(-B // self.shared), self.eta
        counter0 = ((epoch - 1) * self.batches_count + (batch - 1)) * self.n_sides

        def run():
            for sd, side in enumerate(self.sides):
                D.corrupt_codes(G, eta, side, n_choices, self.device, entities_list=entities_list, seed=self.seed,
                                counter=counter0 + sd, out=sl["codes"][sd * eta * G:(sd + 1) * eta * G])

        self._timed("prepare", run)
        sl["key"] = (start, B, epoch, batch)

    def _compute_shared(self, sl, start, B, epoch, batch):
        """forward -> (link) -> loss -> (link) -> backward -> grouping -> apply: the host-driven unfused step with the two shared
        kernels in place of emg_train_forward / emg_train_backward_ex, 2 B + eta_total * G entity gradient rows"""
        pos = self.X[start:start + B]
        Cs, et, eta = self.shared, self.eta_total, self.eta
        G = -(-B // Cs)
        codes = sl["codes"][:G * et]
        n_ce, xe, xr = 2 * B + G * et, self._xe, self._xr
        ce, cr = self.contrib_ent[xe:xe + n_ce], self.contrib_rel[xr:xr + B]
        dest_e, dest_r = sl["dest_ent"][xe:xe + n_ce], sl["dest_rel"][xr:xr + B]
        lr = (sgd_learning_rate(self.sgd_params, self.batches_count, epoch, batch) if self.sgd_params is not None
              else self.lr)
        hyper_e, hyper_r = self._hyper(lr, 0), self._hyper(lr, 1)
        lp_e, lp_r = (self.lp_sum[0:1], self.lp_sum[1:2]) if len(hyper_e) == 8 else (None, None)
        sall = self.scores_all[:B * (1 + et)]
        sp, sn = sall[:B], sall[B:]
        self._timed("forward", lambda: D.shared_forward(self.model_id, self.ent, self.rel, self.k_int, self.scale, pos, Cs, et, codes,
                                                        scores_pos=sp, scores_neg=sn))
        raw_p = raw_n = None
        if self.model_id in (L.TRANSE_L2, L.TRANSE_P):   # the backward takes a triple's norm from its raw score
            raw_p, raw_n = sp, sn
        if self.linked:
            if raw_p is not None:                       # (the link rewrites the scores in place)
                raw = sall.clone()
                raw_p, raw_n = raw[:B], raw[B:]
            fac = self.link_fac[:B * (1 + et)]
            sw = focuse_structure_weight(int(epoch), self.stop_epoch, self.structural_wt) if self.edge_w is not None else 0.0
            ew = self.edge_w[start:start + B] if self.edge_w is not None else None
            D.link_scores(self.link_id, ew, sw, sp, sn, B, et, fac_pos=fac[:B], fac_neg=fac[B:])
        gp, gn = self.g_pos[:B], self.g_neg[:B * et]
        self._timed("loss", lambda: D.loss(self.loss_id, sp, sn, B, eta, self.n_sides, self.margin, self.alpha,
                                           self.loss_accum[0:1], gp, gn))
        if self.linked:
            D.link_grads(gp, gn, fac[:B], fac[B:], B, et)
        self._timed("backward", lambda: D.shared_backward(self.model_id, self.ent, self.rel, self.k_int, self.scale, pos, Cs, et, codes,
                                                          gp, gn, ce, cr, dest_e, dest_r, raw_pos=raw_p, raw_neg=raw_n))

        def group():
            D.group_dest(sl["dest_ent"][:xe + n_ce], xe + n_ce, self.n_ent, sl["ws_ent"])
            D.group_dest(sl["dest_rel"][:xr + B], xr + B, self.n_rel, sl["ws_rel"])

        self._timed("prepare", group)
        self._timed("apply_ent", lambda: D.apply_grouped(self.opt_id, self.ent, self.k_int, self.state_ent[0], self.state_ent[1],
                                                         self.tag_ent, self.step_count, self.contrib_ent[:xe + n_ce], xe + n_ce, False,
                                                         hyper_e, sl["ws_ent"], lp_accum=lp_e))
        self._timed("apply_rel", lambda: D.apply_grouped(self.opt_id, self.rel, self.k_int, self.state_rel[0], self.state_rel[1],
                                                         self.tag_rel, self.step_count, self.contrib_rel[:xr + B], xr + B, False,
                                                         hyper_r, sl["ws_rel"], lp_accum=lp_r))
        if self.normalize:
            D.clip_rows(self.ent, self.k_int, 1.0)

    # ---- relation negatives (DESIGN.md 4.1 "Relation negatives") ----
    def _prepare_relneg(self, sl, start, B, epoch, batch, n_choices, entities_list, inj_mask, inj_repl):
        """The codes of every side under the ordinary step's counters (n_sides counts 'p'): the entity sides as ever, then the
        relation side — emg_corrupt_codes' own draw with the side forced over n_rel - 1 choices, no entity list (the shift past the
        positive's own relation is made by the kernels)"""
        if inj_mask is not None or inj_repl is not None:
            raise ValueError("injected draws are not available with relation negatives")
        eta, n_e = self.eta, self.n_sides - 1
        counter0 = ((epoch - 1) * self.batches_count + (batch - 1)) * self.n_sides
        codes = sl["codes"]

        def run():
            for sd, side in enumerate(self.sides[:n_e]):
                D.corrupt_codes(B, eta, side, n_choices, self.device, entities_list=entities_list, seed=self.seed,
                                counter=counter0 + sd, out=codes[sd * eta * B:(sd + 1) * eta * B])
            D.corrupt_codes(B, eta, L.SIDE_S, self.n_rel - 1, self.device, seed=self.seed, counter=counter0 + n_e,
                            out=codes[n_e * eta * B:(n_e + 1) * eta * B])

        self._timed("prepare", run)
        sl["key"] = (start, B, epoch, batch)

    def _compute_relneg(self, sl, start, B, epoch, batch):
        """forward -> (link) -> loss -> (link) -> backward -> grouping -> apply, host-driven on one stream.  The entity sides (if any)
        go through emg_train_forward / emg_train_backward_ex on their block of the codes; the relation side's two kernels score
        into the last block of scores_neg and append their gradient rows and destinations behind the others."""
        pos = self.X[start:start + B]
        et, eta = self.eta_total, self.eta
        n_e = self.n_sides - 1
        ne = n_e * eta                                   # entity slots per positive
        xe, xr = self._xe, self._xr
        n_ce0 = (2 + ne) * B if n_e else 0               # entity rows of the entity sides
        n_cr0 = B if n_e else 0                          # relation rows of the entity sides (the positives' own)
        n_ce, n_cr = n_ce0 + 2 * B, B + eta * B
        ce, cr = self.contrib_ent[xe:xe + n_ce], self.contrib_rel[xr:xr + n_cr]
        dest_e, dest_r = sl["dest_ent"][xe:xe + n_ce], sl["dest_rel"][xr:xr + n_cr]
        codes_e, codes_p = sl["codes"][:ne * B], sl["codes"][ne * B:et * B]
        lr = (sgd_learning_rate(self.sgd_params, self.batches_count, epoch, batch) if self.sgd_params is not None
              else self.lr)
        hyper_e, hyper_r = self._hyper(lr, 0), self._hyper(lr, 1)
        lp_e, lp_r = (self.lp_sum[0:1], self.lp_sum[1:2]) if len(hyper_e) == 8 else (None, None)
        sall = self.scores_all[:B * (1 + et)]
        sp, sn = sall[:B], sall[B:]
        sn_e, sn_p = sn[:ne * B], sn[ne * B:]

        def forward():
            if n_e:
                D.train_forward(self.model_id, self.ent, self.rel, self.k_int, self.scale, pos, ne, codes_e, scores_pos=sp,
                                scores_neg=sn_e)
            D.relneg_forward(self.model_id, self.ent, self.rel, self.k_int, self.scale, pos, eta, codes_p,
                             scores_pos=None if n_e else sp, scores_neg=sn_p, want_pos=False)

        self._timed("forward", forward)
        raw_p = raw_n = None
        norm = self.model_id in (L.TRANSE_L2, L.TRANSE_P)   # the relation side's backward takes a triple's norm from its raw score
        if norm or (self.wide and self.model_id == L.TRANSE_L2):
            raw_p, raw_n = sp, sn
        if self.linked:
            if raw_p is not None:                       # (the link rewrites the scores in place)
                raw = sall.clone()
                raw_p, raw_n = raw[:B], raw[B:]
            fac = self.link_fac[:B * (1 + et)]
            sw = focuse_structure_weight(int(epoch), self.stop_epoch, self.structural_wt) if self.edge_w is not None else 0.0
            ew = self.edge_w[start:start + B] if self.edge_w is not None else None
            D.link_scores(self.link_id, ew, sw, sp, sn, B, et, fac_pos=fac[:B], fac_neg=fac[B:])
        gp, gn = self.g_pos[:B], self.g_neg[:B * et]
        self._timed("loss", lambda: D.loss(self.loss_id, sp, sn, B, eta, self.n_sides, self.margin, self.alpha,
                                           self.loss_accum[0:1], gp, gn))
        if self.linked:
            D.link_grads(gp, gn, fac[:B], fac[B:], B, et)

        def backward():
            if n_e:
                bw = {}
                if self.wide and self.model_id == L.TRANSE_L2:   # column blocks: the gradient needs the full norm
                    bw = dict(bw_scores_pos=raw_p, bw_scores_neg=raw_n[:ne * B])
                D.train_backward_ex(self.model_id, self.ent, self.rel, self.k_int, self.scale, pos, ne, codes_e, ce[:n_ce0], cr[:B],
                                    fused_loss=-1, g_pos=gp, g_neg=gn[:ne * B], **bw)
                D.build_dest(pos, ne, codes_e, dest_e[:n_ce0], dest_r[:B])
            D.relneg_backward(self.model_id, self.ent, self.rel, self.k_int, self.scale, pos, eta, codes_p, None if n_e else gp,
                              gn[ne * B:], ce[n_ce0:], cr[n_cr0:], dest_e[n_ce0:], dest_r[n_cr0:],
                              raw_pos=None if (n_e or not norm) else raw_p, raw_neg=raw_n[ne * B:] if norm else None)

        self._timed("backward", backward)

        def group():
            D.group_dest(sl["dest_ent"][:xe + n_ce], xe + n_ce, self.n_ent, sl["ws_ent"])
            D.group_dest(sl["dest_rel"][:xr + n_cr], xr + n_cr, self.n_rel, sl["ws_rel"])

        self._timed("prepare", group)
        self._timed("apply_ent", lambda: D.apply_grouped(self.opt_id, self.ent, self.k_int, self.state_ent[0], self.state_ent[1],
                                                         self.tag_ent, self.step_count, self.contrib_ent[:xe + n_ce], xe + n_ce, False,
                                                         hyper_e, sl["ws_ent"], lp_accum=lp_e))
        self._timed("apply_rel", lambda: D.apply_grouped(self.opt_id, self.rel, self.k_int, self.state_rel[0], self.state_rel[1],
                                                         self.tag_rel, self.step_count, self.contrib_rel[:xr + n_cr], xr + n_cr, False,
                                                         hyper_r, sl["ws_rel"], lp_accum=lp_r))
        if self.normalize:
            D.clip_rows(self.ent, self.k_int, 1.0)

    # ---- batch-local regulariser (DESIGN.md 4.1 "Batch regulariser") ----
    def _prepare_batchreg(self, sl, start, B, epoch, batch, n_choices, entities_list, inj_mask, inj_repl):
        """the codes of every side under the ordinary step's counters; destinations and grouping follow the backward (_compute_batchreg)"""
        if inj_mask is not None or inj_repl is not None:
            raise ValueError("injected draws are not available with a batch regulariser")
        eta = self.eta
        counter0 = ((epoch - 1) * self.batches_count + (batch - 1)) * self.n_sides
        codes = sl["codes"]

        def run():
            for sd, side in enumerate(self.sides):
                D.corrupt_codes(B, eta, side, n_choices, self.device, entities_list=entities_list, seed=self.seed,
                                counter=counter0 + sd, out=codes[sd * eta * B:(sd + 1) * eta * B])

        self._timed("prepare", run)
        sl["key"] = (start, B, epoch, batch)

    def _batchreg_rows(self, pos, ce, dest_e, cr, dest_r):
        """emg_batchreg on the positives ``pos``: 2 B entity rows into ``ce`` / ``dest_e``, B relation rows into ``cr`` / ``dest_r``
        unless lambda_rel is zero; R goes to reg_accum (read_loss adds it).  Returns the relation rows written."""
        br = self.batchreg
        B = pos.shape[0]
        has_rel = np.float32(br["lambda_rel"]) != 0 or np.float32(br["lambda_rel"] * br["p"]) != 0
        form = lambda m: L.BATCHREG_MODULUS if m else L.BATCHREG_PLAIN  # noqa: E731
        D.batch_reg(self.ent, self.rel, self.k_int, pos, br["p"], br["lambda_ent"], br["lambda_rel"], form(br["modulus_ent"]),
                    form(br["modulus_rel"]), ce, dest_e[:2 * B], cr if has_rel else None, dest_r[:B] if has_rel else None,
                    value=self.reg_accum)
        return B if has_rel else 0

    def _compute_batchreg(self, sl, start, B, epoch, batch):
        """forward -> (link) -> loss -> (link) -> backward -> destinations -> regulariser rows -> grouping -> apply, host-driven on one
        stream: the ordinary unfused step, with emg_batchreg's 2 B (+ B) gradient rows and destinations appended behind its own."""
        pos = self.X[start:start + B]
        et, eta = self.eta_total, self.eta
        xe, xr = self._xe, self._xr
        n_ce0, n_cr0 = (2 + et) * B, B
        ce, cr = self.contrib_ent[xe:], self.contrib_rel[xr:]
        dest_e, dest_r = sl["dest_ent"][xe:], sl["dest_rel"][xr:]
        codes = sl["codes"][:et * B]
        lr = (sgd_learning_rate(self.sgd_params, self.batches_count, epoch, batch) if self.sgd_params is not None
              else self.lr)
        hyper_e, hyper_r = self._hyper(lr, 0), self._hyper(lr, 1)   # (six values: no folded regulariser)
        sall = self.scores_all[:B * (1 + et)]
        sp, sn = sall[:B], sall[B:]
        self._timed("forward", lambda: D.train_forward(self.model_id, self.ent, self.rel, self.k_int, self.scale, pos, et, codes,
                                                       scores_pos=sp, scores_neg=sn))
        bw = {}
        if self.wide and self.model_id == L.TRANSE_L2:   # column blocks: the gradient needs the full norm, of the RAW scores
            raw = sall.clone() if self.linked else sall  # (the link rewrites the scores in place)
            bw = dict(bw_scores_pos=raw[:B], bw_scores_neg=raw[B:])
        if self.linked:
            fac = self.link_fac[:B * (1 + et)]
            sw = focuse_structure_weight(int(epoch), self.stop_epoch, self.structural_wt) if self.edge_w is not None else 0.0
            ew = self.edge_w[start:start + B] if self.edge_w is not None else None
            D.link_scores(self.link_id, ew, sw, sp, sn, B, et, fac_pos=fac[:B], fac_neg=fac[B:])
        gp, gn = self.g_pos[:B], self.g_neg[:B * et]
        self._timed("loss", lambda: D.loss(self.loss_id, sp, sn, B, eta, self.n_sides, self.margin, self.alpha,
                                           self.loss_accum[0:1], gp, gn))
        if self.linked:
            D.link_grads(gp, gn, fac[:B], fac[B:], B, et)

        def backward():
            D.train_backward_ex(self.model_id, self.ent, self.rel, self.k_int, self.scale, pos, et, codes, ce[:n_ce0], cr[:n_cr0],
                                fused_loss=-1, g_pos=gp, g_neg=gn, **bw)
            D.build_dest(pos, et, codes, dest_e[:n_ce0], dest_r[:n_cr0])

        self._timed("backward", backward)
        n_ce = n_ce0 + 2 * B
        n_cr = n_cr0 + self._timed("batchreg", lambda: self._batchreg_rows(pos, ce[n_ce0:n_ce], dest_e[n_ce0:n_ce], cr[n_cr0:n_cr0 + B],
                                                                         dest_r[n_cr0:n_cr0 + B]))

        def group():
            D.group_dest(sl["dest_ent"][:xe + n_ce], xe + n_ce, self.n_ent, sl["ws_ent"])
            D.group_dest(sl["dest_rel"][:xr + n_cr], xr + n_cr, self.n_rel, sl["ws_rel"])

        self._timed("prepare", group)
        self._timed("apply_ent", lambda: D.apply_grouped(self.opt_id, self.ent, self.k_int, self.state_ent[0], self.state_ent[1],
                                                         self.tag_ent, self.step_count, self.contrib_ent[:xe + n_ce], xe + n_ce, False,
                                                         hyper_e, sl["ws_ent"]))
        self._timed("apply_rel", lambda: D.apply_grouped(self.opt_id, self.rel, self.k_int, self.state_rel[0], self.state_rel[1],
                                                         self.tag_rel, self.step_count, self.contrib_rel[:xr + n_cr], xr + n_cr, False,
                                                         hyper_r, sl["ws_rel"]))
        if self.normalize:
            D.clip_rows(self.ent, self.k_int, 1.0)

    def _compute(self, sl, start, B, epoch, batch, main):
        if self.batchreg is not None:
            return self._compute_batchreg(sl, start, B, epoch, batch)
        if self.shared is not None:
            return self._compute_shared(sl, start, B, epoch, batch)
        if self.relneg:
            return self._compute_relneg(sl, start, B, epoch, batch)
        pos = self.X[start:start + B]
        et, eta = self.eta_total, self.eta
        codes = sl["codes"][:B * et]
        n_ce, n_cr, xe, xr = (2 + et) * B, B, self._xe, self._xr
        ce, cr = self.contrib_ent[xe:xe + n_ce], self.contrib_rel[xr:xr + B]   # batch rows follow the LP rows
        if self.factored:
            ce = self.contrib_ent[:4 * B]
        single = sl["single"][:n_ce] if self.inplace else None
        lr = (sgd_learning_rate(self.sgd_params, self.batches_count, epoch, batch) if self.sgd_params is not None
              else self.lr)
        hyper_e, hyper_r = self._hyper(lr, 0), self._hyper(lr, 1)
        lp_e, lp_r = (self.lp_sum[0:1], self.lp_sum[1:2]) if len(hyper_e) == 8 else (None, None)
        fold = single is not None and len(hyper_e) == 8     # in-place updates fold the regulariser themselves (plain SGD)
        inplace_kw = dict(single_ent=single, opt_id=self.opt_id, step=self.step_count, hyper=hyper_e if fold else hyper_e[:6],
                          ent_state0=self.state_ent[0], ent_state1=self.state_ent[1], tag_ent=self.tag_ent,
                          fac_ws_ent=sl["ws_ent"] if self.factored else None, lp_accum=lp_e if fold else None)
        if self.fused:
            self._timed("fused", lambda: D.train_backward_ex(
                self.model_id, self.ent, self.rel, self.k_int, self.scale, pos, et, codes, ce, cr,
                fused_loss=self.loss_id, margin=self.margin, loss_accum=self.loss_accum, loss_slots=LOSS_SLOTS, **inplace_kw))
        else:
            sall = self.scores_all[:B * (1 + et)]
            sp, sn = sall[:B], sall[B:]
            flags = L.SCORE_PARTIAL if self.sharded else L.SCORE_FINAL
            self._timed("forward", lambda: D.train_forward(self.model_id, self.ent, self.rel, self.k_int, self.scale,
                                                           pos, et, codes, flags=flags, scores_pos=sp, scores_neg=sn))
            bw = {}
            if self.sharded:
                # the ONE collective of a training step: sum the k-slab partial scores over the ranks
                self._timed("allreduce", lambda: (parallel.allreduce_sum_(sall),
                                                  D.finalize_scores(self.model_id, self.scale, sall)))
                if self.model_id == L.TRANSE_L2:  # its gradient needs the full norm, not the slab's
                    bw = dict(bw_scores_pos=sp, bw_scores_neg=sn)
            elif self.wide and self.model_id == L.TRANSE_L2:   # column blocks: the same need
                bw = dict(bw_scores_pos=sp, bw_scores_neg=sn)
            gp, gn = self.g_pos[:B], self.g_neg[:B * et]
            self._timed("loss", lambda: D.loss(self.loss_id, sp, sn, B, eta, self.n_sides, self.margin, self.alpha,
                                               self.loss_accum[0:1], gp, gn))
            self._timed("backward", lambda: D.train_backward_ex(
                self.model_id, self.ent, self.rel, self.k_int, self.scale, pos, et, codes, ce, cr, fused_loss=-1,
                g_pos=gp, g_neg=gn, **bw, **inplace_kw))
        apply_rel = lambda: D.apply_grouped(self.opt_id, self.rel, self.k_int, self.state_rel[0],  # noqa: E731
                                            self.state_rel[1], self.tag_rel, self.step_count, cr, n_cr,
                                            False, hyper_r, sl["ws_rel"], lp_accum=lp_r)
        # (small batches stay on one stream: the fork/join costs ~60 us of host time, more than the overlap buys)
        use_aux = self.aux is not None and n_ce >= AUX_MIN_ROWS
        if use_aux:
            # the relation table's apply (few, long segments: latency-bound, ~0.06 ms at 0.5 TB/s) is independent
            # of the entity table's: it runs on a second stream underneath it
            self.aux_fork.record(main)
            self.aux.wait_event(self.aux_fork)
            with D.on_stream(self.aux):
                self._timed("apply_rel", apply_rel)
                self.aux_join.record(self.aux)
        self._timed("apply_ent", lambda: D.apply_grouped(self.opt_id, self.ent, self.k_int, self.state_ent[0],
                                                         self.state_ent[1], self.tag_ent, self.step_count, ce, n_ce,
                                                         self.inplace, hyper_e, sl["ws_ent"], lp_accum=lp_e,
                                                         factored=self.factored))
        if use_aux:
            main.wait_event(self.aux_join)
        else:
            self._timed("apply_rel", apply_rel)
        if self.normalize:
            # EmbeddingModel.py:1434-1440: tf.clip_by_norm(ent_emb, clip_norm=1, axes=1) after each batch
            D.clip_rows(self.ent, self.k_int, 1.0)

    # ---- batch-sharded step (parallel.py: BATCH sharding) ----
    def _bs_prepare(self, key, n_choices, entities_list, parity):
        """Everything of a batch-sharded step that does not read the tables: this rank's rows of the global batch, their Philox
        negatives and local grouping (emg_prepare_batch) and — device exchange — the exchange's metadata phase for both tables.
        Issued on the side stream a step ahead when the caller names the next batch (``prefetch``)."""
        start, B, epoch, batch = key
        rank, world = parallel.rank_world()
        r0, r1 = parallel.batch_rows(B, rank, world)
        Bl = r1 - r0
        et, eta = self.eta_total, self.eta
        n_ce = (2 + et) * Bl
        st = {"key": key, "parity": parity, "r0": r0, "Bl": Bl, "n_ce": n_ce, "pe": None, "pr": None}
        dev = self.device
        if Bl > 0:
            self._alloc_scratch(Bl)
        sl = self.slots[parity % len(self.slots)]
        if Bl > 0:
            pos = self.X[start + r0:start + r1]
            counter0 = ((epoch - 1) * self.batches_count + (batch - 1)) * self.n_sides
            D.prepare_batch(pos, eta, self.sides, self.n_ent if n_choices is None else int(n_choices), sl["codes"][:Bl * et],
                            sl["dest_ent"][:n_ce], sl["dest_rel"][:Bl], self.n_ent, self.n_rel, sl["ws_ent"], sl["ws_rel"],
                            entities_list=entities_list, seed=self.seed, counter0=counter0, B_global=B, row_offset=r0)
        if self._device_exchange:
            if Bl > 0:
                gslot_e, gslot_r = self._gslots(Bl, B, r0, n_ce)      # slot of the same row in the whole batch's layout
                sorted_e = D.apply_workspace_views(sl["ws_ent"], n_ce)   # the local grouping: destinations ascending, slots in order
                sorted_r = D.apply_workspace_views(sl["ws_rel"], Bl)
            else:
                z32 = torch.zeros(0, dtype=torch.int32, device=dev)
                gslot_e = gslot_r = z32
                sorted_e = sorted_r = (z32, z32)
            st["pe"] = self._plan_exchange("ent", sorted_e[0], sorted_e[1], gslot_e, parity)
            st["pr"] = self._plan_exchange("rel", sorted_r[0], sorted_r[1], gslot_r, parity)
        return st

    def _step_batch_sharded(self, start, B, epoch, batch, n_choices, entities_list, prefetch=None):
        """[start, start + B) is the GLOBAL batch.  This rank scores rows [r0, r1) of it with the negatives the whole batch draws
        for them, then: gradient rows -> owners (all_to_all) -> one summed row per destination, added in global slot order ->
        all-gather -> every replica applies the optimizer (parallel.py: BATCH sharding).  Device exchange (default): the
        table-independent half — preparation, row counts, (destination, slot) pairs, groupings — is issued for the NEXT batch on a
        side stream as soon as this step's kernels are enqueued; between the scoring kernel and the apply there is no host read."""
        key = (start, B, epoch, batch)
        self.step_count += 1
        et, eta, k = self.eta_total, self.eta, self.k_int
        lr = (sgd_learning_rate(self.sgd_params, self.batches_count, epoch, batch) if self.sgd_params is not None
              else self.lr)
        dev = self.device
        main = torch.cuda.current_stream()
        st = self._bs_ready.pop(key, None)
        if st is None:
            self._bs_ready.clear()                 # (a prefetch list that did not match the steps: nothing prepared is kept)
            st = self._bs_prepare(key, n_choices, entities_list, self._bs_parity)
        else:
            main.wait_event(st["event"])           # the side stream's preparation and metadata phase of this batch
        self._bs_parity = st["parity"] ^ 1
        Bl, r0, n_ce = st["Bl"], st["r0"], st["n_ce"]
        sl = self.slots[st["parity"] % len(self.slots)]
        if Bl > 0:
            pos = self.X[start + r0:start + r0 + Bl]
            codes = sl["codes"][:Bl * et]
            ce, cr = self.contrib_ent[:n_ce], self.contrib_rel[:Bl]
            if self.fused:
                D.train_backward_ex(self.model_id, self.ent, self.rel, k, self.scale, pos, et, codes, ce, cr,
                                    fused_loss=self.loss_id, margin=self.margin, loss_accum=self.loss_accum, loss_slots=LOSS_SLOTS)
            else:
                sall = self.scores_all[:Bl * (1 + et)]
                sp, sn = sall[:Bl], sall[Bl:]
                D.train_forward(self.model_id, self.ent, self.rel, k, self.scale, pos, et, codes, scores_pos=sp, scores_neg=sn)
                gp, gn = self.g_pos[:Bl], self.g_neg[:Bl * et]
                D.loss(self.loss_id, sp, sn, Bl, eta, self.n_sides, self.margin, self.alpha, self.loss_accum[0:1], gp, gn)
                D.train_backward_ex(self.model_id, self.ent, self.rel, k, self.scale, pos, et, codes, ce, cr, fused_loss=-1,
                                    g_pos=gp, g_neg=gn)
            dest_e, dest_r = sl["dest_ent"][:n_ce], sl["dest_rel"][:Bl]
            rows_e, rows_r = ce, cr
        else:
            dest_e = dest_r = torch.zeros(0, dtype=torch.int32, device=dev)
            rows_e = rows_r = torch.zeros((0, k), dtype=torch.float32, device=dev)
        lp = (self.lp_sum[0:1], self.lp_sum[1:2]) if self.reg is not None else (None, None)
        he, hr = self._hyper(lr, 0), self._hyper(lr, 1)
        if self._device_exchange:
            # data phase: rows -> owners, summed in global slot order, sums -> every replica, optimizer
            self._exchange_apply_planned("ent", st["pe"], rows_e, self.ent, self.state_ent, self.tag_ent, he, lp[0], st["parity"])
            self._exchange_apply_planned("rel", st["pr"], rows_r, self.rel, self.state_rel, self.tag_rel, hr, lp[1], st["parity"])
        else:
            if Bl > 0:
                gslot_e, gslot_r = self._gslots(Bl, B, r0, n_ce)
            else:
                gslot_e = gslot_r = dest_e
            self._exchange_apply(self.ent, self.n_ent, self.state_ent, self.tag_ent, dest_e, gslot_e.to(torch.int64), rows_e, he, "ent", lp[0])
            self._exchange_apply(self.rel, self.n_rel, self.state_rel, self.tag_rel, dest_r, gslot_r.to(torch.int64), rows_r, hr, "rel", lp[1])
        if self.normalize:
            D.clip_rows(self.ent, k, 1.0)
        self._bs_done[st["parity"]].record(main)
        # the next batch's table-independent half, on the side stream, now: it runs beside this step's exchange and apply
        if self._bs_ahead and prefetch:
            nxt = prefetch if isinstance(prefetch, tuple) else next((p for p in prefetch if p is not None and p[1] > 0), None)
            if nxt is not None and tuple(nxt[:4]) not in self._bs_ready:
                par = st["parity"] ^ 1
                side = self._bs_stream
                side.wait_event(self._bs_done[par])          # the step that last used that slot and those workspaces (two steps back)
                with torch.cuda.stream(side):
                    nst = self._bs_prepare(tuple(nxt[:4]), nxt[4] if len(nxt) > 4 else n_choices, nxt[5] if len(nxt) > 5 else entities_list, par)
                    nst["event"] = torch.cuda.Event()
                    nst["event"].record(side)
                for pl in (nst["pe"], nst["pr"]):            # (allocated on the side stream, read by the main stream's data phase)
                    if pl is not None:
                        pl.order.record_stream(main)
                        pl.uniq_local.record_stream(main)
                self._bs_ready[tuple(nxt[:4])] = nst

    def _gslots(self, Bl, B, r0, n_ce):
        """global contribution slot of every local slot (int32): local slot t = role block t // Bl, row t % Bl -> block * B + r0 + row"""
        key = (Bl, B, r0, n_ce)
        if self._gslot_cache.get("key") != key:
            t = torch.arange(n_ce, dtype=torch.int64, device=self.device)
            self._gslot_cache = {"key": key, "e": ((t // Bl) * B + r0 + (t % Bl)).to(torch.int32),
                                 "r": (r0 + torch.arange(Bl, dtype=torch.int64, device=self.device)).to(torch.int32)}
        return self._gslot_cache["e"], self._gslot_cache["r"]

    def _xchg(self, which):
        x = self._xchg_objs.get(which)
        if x is None:
            x = parallel.RowExchange(self.n_ent if which == "ent" else self.n_rel, self.k_int, self.device)
            x.sums = alloc_table(max(1, x.e1 - x.e0), self.k_int, self.device)   # this rank's range: one summed gradient row per owned row
            x.compact = None
            x.ws_owner, x.ws_rep = [None, None], [None, None]
            self._xchg_objs[which] = x
        return x

    @staticmethod
    def _grown(buf, need, device):
        if buf is None or buf.numel() < need:
            return torch.empty(int(need * 1.25) + 1024, dtype=torch.uint8, device=device)
        return buf

    def _plan_exchange(self, which, dest_sorted, order, gslot, parity=0):
        """METADATA phase of one table's exchange (parallel.RowExchange): nothing here reads the tables.  The two grouping
        workspaces exist twice (``parity``): the next batch's are filled while this batch's are being applied from."""
        x, k = self._xchg(which), self.k_int
        pl = x.plan_counts(dest_sorted, order, gslot)
        owned = max(1, x.e1 - x.e0)
        if pl.m:
            # the owner's order: by destination, a destination's rows in GLOBAL slot order (the order one GPU adds them in)
            x.ws_owner[parity] = self._grown(x.ws_owner[parity], D.apply_workspace_bytes(pl.m, owned, k), self.device)
            D.group_dest_keyed(pl.dest_o, pl.gslot_o, pl.m, owned, x.ws_owner[parity])
            keys_o = D.apply_workspace_views(x.ws_owner[parity], pl.m)[0]
        else:
            keys_o = pl.dest_o
        x.plan_unique(pl, keys_o)
        n_all = x.world * pl.cap_u
        x.ws_rep[parity] = self._grown(x.ws_rep[parity], D.apply_workspace_bytes(n_all, x.n_rows, k), self.device)
        D.group_dest(pl.ids_all, n_all, x.n_rows, x.ws_rep[parity])        # (the sentinel ids of the padding are dropped: no row to update)
        return pl

    def _exchange_apply_planned(self, which, pl, rows, table, state, tag, hyper, lp_accum, parity=0):
        """DATA phase: gradient rows -> owners (all_to_all) -> one summed row per destination, added in global slot order ("SGD with
        lr = -1 on a zero row" is 0 - (-1 * g) = g exactly: emg_apply_grouped as a segmented sum) -> all-gather -> every replica
        applies the optimizer to the same sums with its own (replicated, hence identical) state"""
        x, k = self._xchg(which), self.k_int
        recv = x.send_rows(pl, rows)
        x.sums.index_fill_(0, pl.uniq_local, 0.0)
        if pl.m:
            D.apply_grouped(L.OPT_SGD, x.sums, k, None, None, None, 1, recv, pl.m, False, (-1.0, 0, 0, 0, 0, 0), x.ws_owner[parity], factored=True)
        if x.compact is None or x.compact.shape[0] < pl.cap_u:
            x.compact = torch.empty((int(pl.cap_u * 1.25) + 64, k), dtype=torch.float32, device=self.device)
        comp = x.compact[:pl.cap_u]
        torch.index_select(x.sums, 0, pl.uniq_local, out=comp)
        if self.shard_state:
            # the OWNER applies the optimizer to its rows (its shard of the state), the UPDATED rows are all-gathered and every
            # replica copies them into its table: one update per touched row in the whole job instead of one per replica
            own = table[x.e0:x.e1]
            dest_local = torch.where(pl.mine < x.n_rows, pl.mine - x.e0, torch.full_like(pl.mine, x.e1 - x.e0))   # padding: outside the range
            x.ws_own = self._grown(getattr(x, "ws_own", None), D.apply_workspace_bytes(pl.cap_u, max(1, x.e1 - x.e0), k), self.device)
            D.apply_rows(self.opt_id, own, k, state[0], state[1], None, self.step_count, comp, dest_local, pl.cap_u, hyper, x.ws_own)
            torch.index_select(own[:, :k], 0, pl.uniq_local, out=comp)          # (padding entries: row 0 of the range; their ids are skipped)
            g = x.gather_sums(pl, comp)
            D.scatter_rows(table, k, g, pl.ids_all)
            self.opt_rows += pl.rows_mine
        else:
            g = x.gather_sums(pl, comp)
            D.apply_grouped(self.opt_id, table, k, state[0], state[1], tag, self.step_count, g, x.world * pl.cap_u, False, hyper, x.ws_rep[parity],
                            lp_accum=lp_accum)
            self.opt_rows += pl.rows_all
        self.opt_rows_owner_form += pl.rows_mine
        self.opt_rows_replicated_form += pl.rows_all
        self.xgmi_bytes += pl.sent_bytes + pl.recv_bytes

    def _exchange_apply(self, table, n_rows, state, tag, dest, gslot, rows, hyper, which, lp_accum=None):
        """gradient rows -> owners (all_to_all) -> per destination ONE summed row, added in global slot order (the order a
        single GPU adds them in) -> all-gather of (destination, summed row) -> every replica applies the optimizer to the
        same sums with its own (replicated, hence identical) state: tables, state and loss are those of one GPU, bit for
        bit, for every optimizer — Keras Adam's dense decay and a folded LP regulariser included (they need every row)."""
        k = self.k_int
        dest_o, gslot_o, rows_o, sent = parallel.exchange_rows(dest, gslot, rows, n_rows)
        m = int(dest_o.numel())
        if m:
            # the sum order: by slot of the (global) batch layout; the stable grouping by destination below keeps it.
            # Destinations are renumbered 0..u-1 so that the sums land in a compact [u, k] buffer: "SGD with lr = -1 on a
            # zero table" is 0 - (-1 * g) = g exactly, i.e. emg_apply_grouped used as a segmented sum
            perm = torch.argsort(gslot_o, stable=True)
            dest_p = dest_o.index_select(0, perm)
            upd, compact = torch.unique(dest_p, sorted=True, return_inverse=True)
            u = int(upd.numel())
            ws = self._owner_ws.get(which)
            need = D.apply_workspace_bytes(m, u, k)
            if ws is None or ws.numel() < need:
                ws = self._owner_ws[which] = torch.empty(int(need * 1.5) + 1024, dtype=torch.uint8, device=self.device)
            cid = compact.to(torch.int32).contiguous()
            D.group_dest(cid, m, u, ws)
            keys, vals = D.apply_workspace_views(ws, m)
            vals.copy_(perm.index_select(0, vals.to(torch.int64)).to(torch.int32))   # positions in RECEIVE order
            sums = alloc_table(u, k, self.device)        # (zero-filled)
            D.apply_grouped(L.OPT_SGD, sums, k, None, None, None, 1, rows_o, m, False, (-1.0, 0, 0, 0, 0, 0), ws)
            upd = upd.to(torch.int32)
        else:
            upd = torch.zeros(0, dtype=torch.int32, device=self.device)
            sums = alloc_table(1, k, self.device)[:0]
        oid, orow, recvd = parallel.allgather_rows(upd, sums)
        ids = torch.cat([upd, oid]) if oid.numel() else upd
        g = torch.cat([sums, orow.to(sums.dtype)]) if oid.numel() else sums
        n = int(ids.numel())
        # every replica: one optimizer step per touched row from its summed gradient (each destination occurs once: a
        # segment of one row), the dense pass for the rest where the optimizer / regulariser needs one
        ws2 = self._owner_ws.get(which + "2")
        need2 = D.apply_workspace_bytes(max(n, 1), n_rows, k)
        if ws2 is None or ws2.numel() < need2:
            ws2 = self._owner_ws[which + "2"] = torch.empty(int(need2 * 1.5) + 1024, dtype=torch.uint8, device=self.device)
        gg = alloc_table(max(n, 1), k, self.device)
        if n:
            gg[:n].copy_(g)
            D.group_dest(ids.contiguous(), n, n_rows, ws2)
        D.apply_grouped(self.opt_id, table, k, state[0], state[1], tag, self.step_count, gg, n, False, hyper, ws2, lp_accum=lp_accum)
        self.xgmi_bytes += sent + recvd

    def read_loss(self, reset=True):
        """data loss (identical on every rank) + LP term (summed over the column slabs when sharded)"""
        if self.deferred and self.reg is not None:
            self.materialize()   # the regulariser's value over the rows whose dense updates are still pending
        reg, data = self.reg_accum, self.loss_accum
        if self.sharded:  # sum a COPY over the ranks: the accumulator itself stays rank-local (reset=False calls)
            reg = parallel.allreduce_sum_(self.reg_accum.clone())
        if self.batch_sharded:  # every rank saw its rows of each batch only; the LP term was computed by every replica
            data = parallel.allreduce_sum_(self.loss_accum.clone())
        v = float(data.sum().item()) + float(reg.item())
        if self.reg is not None:   # (batch-sharded: every replica folded the regulariser over the full tables itself)
            lp = self.lp_sum if not self.sharded else parallel.allreduce_sum_(self.lp_sum.clone())
            lp = lp.cpu()
            v += self.reg[0] * float(lp[0]) + self.reg[1] * float(lp[1])
        if reset:
            self.loss_accum.zero_()
            self.reg_accum.zero_()
            self.lp_sum.zero_()
        return v

    def _step_lr(self, t):
        """the learning rate optimizer step t uses (Adam: lr_t), assuming fit()'s order of batches (step t = batch (t - 1) mod
        batches_count of epoch (t - 1) // batches_count); a step issued out of that order corrects its own entry"""
        if self.opt_id == L.OPT_ADAM:
            return self.lr * math.sqrt(1.0 - ADAM_BETA2 ** t) / (1.0 - ADAM_BETA1 ** t)
        if self.sgd_params is not None:
            return sgd_learning_rate(self.sgd_params, self.batches_count, (t - 1) // self.batches_count + 1, (t - 1) % self.batches_count + 1)
        return self.lr

    LR_TABLE_STEPS = 1 << 22    # entries of the deferred pass's learning-rate table (16 MB)

    def _deferred_table_check(self, n_more):
        """the deferred pass reads each replayed step's learning rate from a table of LR_TABLE_STEPS entries the plan points at; a
        fit that long (e.g. batches_count = 1000 for 4200 epochs) brings every row up to date once and goes on with the dense pass"""
        if self.deferred and self._lr_t_hist is not None and self.step_count + n_more >= self._lr_t_hist.numel():
            self.materialize()
            self.deferred = False
            self._make_plan()

    def _fill_lr_t(self, upto, lr_now=None):
        """learning rates of the steps (filled, upto] into the device table the replay reads: the values _hyper hands the
        kernels, float32-rounded the same way; ``lr_now``: what step ``upto`` really uses"""
        if upto >= self._lr_t_hist.numel():
            raise RuntimeError("deferred dense pass: more than %d optimizer steps" % self._lr_t_hist.numel())
        if upto > self._lr_t_filled:
            hi = min(max(upto, self._lr_t_filled + 8192), self._lr_t_hist.numel() - 1)   # ahead in blocks: one upload per 8192 steps
            vals = [self._step_lr(t) for t in range(self._lr_t_filled + 1, hi + 1)]
            self._lr_host.extend(np.asarray(vals, dtype=np.float64).astype(np.float32).tolist())
            self._lr_t_hist[self._lr_t_filled + 1:hi + 1] = torch.tensor(vals, dtype=torch.float64).to(torch.float32).to(self.device)
            self._lr_t_filled = hi
        if lr_now is not None and self.opt_id != L.OPT_ADAM:
            v = float(np.float32(lr_now))
            if self._lr_host[upto] != v:      # a step outside fit()'s order (tests drive epochs / batches freely)
                self._lr_host[upto] = v
                self._lr_t_hist[upto:upto + 1] = torch.tensor([lr_now], dtype=torch.float64).to(torch.float32).to(self.device)

    def materialize(self):
        """deferred dense pass: bring every row of both tables (and its optimizer state) up to the current step"""
        if not self.deferred or self.step_count == 0 or self._lr_t_hist is None:
            return
        import ctypes as C
        lib = L.load()
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        for i, (tab, n, state, tag) in enumerate(((self.ent, self.n_ent, self.state_ent, self.tag_ent),
                                                  (self.rel, self.n_rel, self.state_rel, self.tag_rel))):
            hy = self._hyper(self.lr, i)
            h = (C.c_float * 8)(*(hy if len(hy) == 8 else hy + (0.0, 0.0)))
            lp = self.lp_sum[i:i + 1].data_ptr() if self.reg is not None else None
            L.check(lib.emg_deferred_materialize(self.opt_id, tab.data_ptr(), n, tab.stride(0), self.k_int, ptr(state[0]), ptr(state[1]),
                                                 tag.data_ptr(), h, self._lr_t_hist.data_ptr(), self.step_count, lp, st),
                    "emg_deferred_materialize")

    def tables_numpy(self):
        self.materialize()
        # (.cpu() of a device tensor is a fresh host copy already; only padded rows need compacting)
        return np.ascontiguousarray(self.ent.cpu().numpy()), np.ascontiguousarray(self.rel.cpu().numpy())
