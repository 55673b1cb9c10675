"""Host side of the filtered 1-vs-all ranking path (mirrors emgraph/evaluation/protocol.py and the
eval half of emgraph/models/EmbeddingModel.py).

What stays on the host (numpy, vectorised — no SQLite, no per-triple Python):
  * the filter index: a one-off CSR of known positives per (query, side), replacing
    SQLiteAdapter.get_participating_entities (sqlite_adapter.py:449-508: two SQL queries + a connect per
    test triple);
  * turning the device's (gt, eq) counters into ranks (perform_comparision's three strategies,
    EmbeddingModel.py:2010-2033, and the rank assembly :1966-1986).
Everything numeric runs in libemgraph_hip.so.
"""
from __future__ import annotations


import math
import typing

import numpy as np
import torch

from .. import _lib as L
from .. import _switches
from .. import device as D


def _expand_ranges(lo, hi):
    """indices of concatenated ranges [lo_i, hi_i) + the owning range id of each index"""
    lens = (hi - lo).astype(np.int64)
    total = int(lens.sum())
    owner = np.repeat(np.arange(len(lo), dtype=np.int64), lens)
    if total == 0:
        return np.zeros(0, np.int64), owner
    starts = np.cumsum(lens) - lens
    idx = np.arange(total, dtype=np.int64) - np.repeat(starts, lens) + np.repeat(lo.astype(np.int64), lens)
    return idx, owner


def _stable_argsort(key):
    """stable argsort of non-negative int64 keys.  Large key sets that fit 31 bits go through the library's stable radix
    sort on the GPU (emg_group_dest: the grouping the training step uses; 1M keys in well under a millisecond + two 4 MB
    copies, against ~75 ms for numpy's merge sort); anything else — small sets, wide keys, a GPU-less host — through numpy.
    Both orders are THE stable order, so the index is the same either way."""
    n = len(key)
    if n >= 100_000 and torch.cuda.is_available() and int(key.max()) < (1 << 31) - 1 and int(key.min()) >= 0:
        dev = torch.device("cuda", torch.cuda.current_device())
        # on its own stream: the index is built lazily, i.e. usually while the big count kernel of the first query tile
        # runs on the caller's stream — the sort must not queue behind it
        side = _sort_streams.get(dev.index)
        if side is None:
            side = _sort_streams[dev.index] = torch.cuda.Stream(device=dev, priority=-1)
        with torch.cuda.stream(side):
            kd = torch.from_numpy(key.astype(np.int32)).to(dev)
            ws = torch.empty(D.apply_workspace_bytes(n, int(key.max()) + 1), dtype=torch.uint8, device=dev)
            D.group_dest(kd, n, int(key.max()) + 1, ws)
            order = D.apply_workspace_views(ws, n)[1].cpu().numpy().astype(np.int64)   # (synchronises the side stream only)
        return order
    return np.argsort(key, kind="stable")


_sort_streams = {}


class FilterIndex:
    """One-off index of the filter triples: (s,p)-sorted objects and (o,p)-sorted subjects.  Built once
    per evaluate_performance call (two argsorts); each query chunk then costs two searchsorted calls.
    Replaces the SQLite side-table + its (subject,predicate) / (predicate,object) indexes
    (sqlite_adapter.py:54-98,234-262) and the two SQL queries + connect per test triple (:449-508)."""

    def __init__(self, filter_triples):
        F = np.asarray(filter_triples, dtype=np.int64).reshape(-1, 3)
        self.n_rel = int(F[:, 1].max()) + 1 if len(F) else 1
        self.max_entity = int(max(F[:, 0].max(), F[:, 2].max())) if len(F) else -1
        self._F = F
        self._Fd = None
        self._cols = None
        self._sides = {}     # built on first use (_side): rank_triples_device asks for the CSR of a query tile AFTER it has
                             # launched the tile's count kernel, so the two sorts run underneath that kernel

    def _side(self, name):
        """(sorted keys, values in that order) of one side: 'obj' = objects by (subject, relation), 'sub' = subjects by
        (object, relation)"""
        if name not in self._sides:
            kcol, vcol = {"obj": (0, 2), "sub": (2, 0)}[name]
            n, kmax = len(self._F), (self.max_entity + 1) * self.n_rel
            if n >= 100_000 and torch.cuda.is_available() and 0 <= kmax < (1 << 31) - 1 and int(self._F.min()) >= 0:
                # large filter sets on a GPU host: keys, the stable sort (the library's grouping) and the two gathers on the
                # device, on a stream of their own (usually underneath the count kernel of the first query tile)
                dev = torch.device("cuda", torch.cuda.current_device())
                side = _sort_streams.get(dev.index)
                if side is None:
                    side = _sort_streams[dev.index] = torch.cuda.Stream(device=dev, priority=-1)
                with torch.cuda.stream(side):
                    if self._Fd is None:
                        self._Fd = torch.from_numpy(self._F).to(dev)
                    key = self._Fd[:, kcol] * self.n_rel + self._Fd[:, 1]
                    ws = torch.empty(D.apply_workspace_bytes(n, kmax + 1), dtype=torch.uint8, device=dev)
                    D.group_dest(key.to(torch.int32), n, kmax + 1, ws)
                    order = D.apply_workspace_views(ws, n)[1].long()
                    self._sides[name] = (key.index_select(0, order).cpu().numpy(),
                                         self._Fd[:, vcol].index_select(0, order).cpu().numpy())
                if len(self._sides) == 2:
                    self._Fd = None
                return self._sides[name]
            if self._cols is None:   # contiguous columns: the strided [n, 3] views cost 3-4x in every pass below
                self._cols = [np.ascontiguousarray(self._F[:, c]) for c in range(3)]
            key = self._cols[kcol] * self.n_rel + self._cols[1]
            order = _stable_argsort(key)
            self._sides[name] = (key[order], self._cols[vcol][order])
        return self._sides[name]

    def _pairs(self, name, q_ent, q_rel, q_self):
        """(row, entity) pairs: filter entities matching the row's (entity, relation) key, plus the row's
        own entity ('select <id> union select distinct ...', sqlite_adapter.py:472-495)."""
        skey, sval = self._side(name)
        qk = np.where(q_rel < self.n_rel, q_ent * self.n_rel + q_rel, -1)
        lo = np.searchsorted(skey, qk, side="left")
        hi = np.searchsorted(skey, qk, side="right")
        idx, owner = _expand_ranges(lo, hi)
        rows = np.concatenate([owner, np.arange(len(qk), dtype=np.int64)])
        ents = np.concatenate([sval[idx], q_self.astype(np.int64)])
        return rows, ents

    def csr(self, test_triples, side_mode, n_ent, entities_subset=None):
        """CSR (filt_ptr int64[n_rows+1], filt_idx int32) of known positives per query ROW, in the row
        order of emg_eval_build_queries (object-side rows first for 's+o'/'s,o').

        object-side row of (s,p,o):  {o} U {o' : (s,p,o') in F};  subject-side: {s} U {s' : (s',p,o) in F}.
        With ``entities_subset`` only members of the subset are kept (EmbeddingModel.py:1898-1940 intent)."""
        T = np.asarray(test_triples, dtype=np.int64).reshape(-1, 3)
        n_q = T.shape[0]
        rows_all, ents_all = [], []
        row_base = 0
        if side_mode in (L.EVAL_O, L.EVAL_SPO, L.EVAL_S_O):
            r, e = self._pairs("obj", T[:, 0], T[:, 1], T[:, 2])
            rows_all.append(r + row_base)
            ents_all.append(e)
            row_base += n_q
        if side_mode in (L.EVAL_S, L.EVAL_SPO, L.EVAL_S_O):
            r, e = self._pairs("sub", T[:, 2], T[:, 1], T[:, 0])
            rows_all.append(r + row_base)
            ents_all.append(e)
            row_base += n_q
        n_rows = row_base
        rows = np.concatenate(rows_all) if rows_all else np.zeros(0, np.int64)
        ents = np.concatenate(ents_all) if ents_all else np.zeros(0, np.int64)
        if entities_subset is not None:
            keep = np.isin(ents, np.asarray(entities_subset, dtype=np.int64))
            rows, ents = rows[keep], ents[keep]
        comb = np.unique(rows * np.int64(n_ent) + ents)  # de-duplicate (SQL UNION / DISTINCT), sorted by row
        rows_u = comb // n_ent
        ents_u = (comb - rows_u * n_ent).astype(np.int32)
        ptr = np.zeros(n_rows + 1, np.int64)
        np.cumsum(np.bincount(rows_u, minlength=n_rows), out=ptr[1:])
        return ptr, ents_u


    def known_csr(self, queries, side, n_ent, entities_subset=None):
        """CSR (ptr int64[n + 1], idx int32 ascending per row) of the KNOWN completions of n queries, from the same sorted
        sides as `csr` but without a row's own entity (a top-N query has none):
        side 'o', row (s, p): {o' : (s, p, o') in F};  side 's', row (p, o): {s' : (s', p, o) in F}.
        With ``entities_subset`` only members of the subset are kept."""
        if side not in ("s", "o"):
            raise ValueError("side must be 's' or 'o'")
        q = np.asarray(queries, dtype=np.int64).reshape(-1, 2)
        q_ent, q_rel = (q[:, 0], q[:, 1]) if side == "o" else (q[:, 1], q[:, 0])
        skey, sval = self._side("obj" if side == "o" else "sub")
        qk = np.where((q_rel >= 0) & (q_rel < self.n_rel), q_ent * self.n_rel + q_rel, -1)
        idx, rows = _expand_ranges(np.searchsorted(skey, qk, side="left"), np.searchsorted(skey, qk, side="right"))
        ents = sval[idx].astype(np.int64)
        if entities_subset is not None:
            keep = np.isin(ents, np.asarray(entities_subset, dtype=np.int64))
            rows, ents = rows[keep], ents[keep]
        comb = np.unique(rows * np.int64(n_ent) + ents)   # distinct, by row, ascending ids within a row
        rows_u = comb // n_ent
        ptr = np.zeros(len(q) + 1, np.int64)
        np.cumsum(np.bincount(rows_u, minlength=len(q)), out=ptr[1:])
        return ptr, (comb - rows_u * n_ent).astype(np.int32)


    # ---- relation side: the relations known between a (subject, object) pair ----
    def _rel_side(self):
        """(sorted keys s * (max_entity + 1) + o, relations in that order), built on first use like `_side`"""
        if "rel" not in self._sides:
            n_key = self.max_entity + 1
            if n_key * n_key >= (1 << 63):
                raise NotImplementedError("the filter's entity ids are too large for a 64-bit (subject, object) key")
            if self._cols is None:
                self._cols = [np.ascontiguousarray(self._F[:, c]) for c in range(3)]
            key = self._cols[0] * np.int64(max(n_key, 1)) + self._cols[2]
            order = np.argsort(key, kind="stable")
            self._sides["rel"] = (key[order], self._cols[1][order])
        return self._sides["rel"]

    def _known_rels(self, q_s, q_o, n_rel, relations_subset):
        """(row, relation) of every filter triple (s, p', o) of the rows' pairs, p' in [0, n_rel) (and in the subset)"""
        skey, sval = self._rel_side()
        n_key = self.max_entity + 1
        seen = (q_s >= 0) & (q_s < n_key) & (q_o >= 0) & (q_o < n_key)
        qk = np.where(seen, q_s * np.int64(max(n_key, 1)) + q_o, -1)
        idx, rows = _expand_ranges(np.searchsorted(skey, qk, side="left"), np.searchsorted(skey, qk, side="right"))
        rels = sval[idx].astype(np.int64)
        keep = (rels >= 0) & (rels < n_rel)
        if relations_subset is not None:
            keep &= np.isin(rels, np.asarray(relations_subset, dtype=np.int64))
        return rows[keep], rels[keep]

    @staticmethod
    def _rel_rows_csr(rows, rels, n_rows, n_rel):
        comb = np.unique(rows * np.int64(n_rel) + rels)   # distinct, by row, ascending ids within a row
        rows_u = comb // n_rel
        ptr = np.zeros(n_rows + 1, np.int64)
        np.cumsum(np.bincount(rows_u, minlength=n_rows), out=ptr[1:])
        return ptr, (comb - rows_u * n_rel).astype(np.int32)

    def rel_csr(self, test_triples, n_rel, relations_subset=None):
        """CSR (ptr int64[n + 1], idx int32 ascending per row) of the relation-side filter set of every test triple (s, p, o):
        {p} U {p' : (s, p', o) in F}.  With ``relations_subset`` only its members are kept of the known relations; the row's own
        p always stays (a p outside the candidates is never met by the count's membership test)."""
        T = np.asarray(test_triples, dtype=np.int64).reshape(-1, 3)
        if T.size and not ((T[:, 1] >= 0) & (T[:, 1] < n_rel)).all():
            raise ValueError("test_triples holds a relation id outside [0, %d)" % n_rel)
        rows, rels = self._known_rels(T[:, 0], T[:, 2], n_rel, relations_subset)
        rows = np.concatenate([rows, np.arange(len(T), dtype=np.int64)])
        rels = np.concatenate([rels, T[:, 1]])
        return self._rel_rows_csr(rows, rels, len(T), n_rel)

    def known_rel_csr(self, pairs, n_rel, relations_subset=None):
        """CSR (ptr int64[n + 1], idx int32 ascending per row) of the KNOWN relations of n (subject, object) pairs:
        {p' : (s, p', o) in F}, with ``relations_subset`` its members only."""
        q = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        rows, rels = self._known_rels(q[:, 0], q[:, 1], n_rel, relations_subset)
        return self._rel_rows_csr(rows, rels, len(q), n_rel)


def build_filter_csr(filter_triples, test_triples, side_mode, n_ent, entities_subset=None):
    """Convenience: FilterIndex(filter_triples).csr(...)."""
    return FilterIndex(filter_triples).csr(test_triples, side_mode, n_ent, entities_subset)


def _cmp(gt, eq, strategy):
    """perform_comparision (EmbeddingModel.py:2018-2033) from the (>, ==) counters."""
    if strategy == "worst":
        return gt + eq
    if strategy == "best":
        return gt
    if strategy == "middle":
        return gt + np.ceil(eq / 2).astype(np.int64)
    raise AssertionError("Invalid score comparision type!")


def ranks_from_counts(gt, eq, fgt, feq, n_q, corrupt_side, strategy):
    """rank assembly (EmbeddingModel.py:1966-1986).  's,o' -> [n,2] = [subject_rank, object_rank]."""
    gt, eq, fgt, feq = [np.asarray(a, dtype=np.int64) for a in (gt, eq, fgt, feq)]
    if corrupt_side in ("s", "o"):
        return _cmp(gt, eq, strategy) + 1 - _cmp(fgt, feq, strategy)
    o, s = slice(0, n_q), slice(n_q, 2 * n_q)
    if corrupt_side == "s,o":
        rank_s = _cmp(gt[s], eq[s], strategy) + 1 - _cmp(fgt[s], feq[s], strategy)
        rank_o = _cmp(gt[o], eq[o], strategy) + 1 - _cmp(fgt[o], feq[o], strategy)
        return np.stack([rank_s, rank_o], axis=1)
    if corrupt_side == "s+o":
        return (_cmp(gt[o] + gt[s], eq[o] + eq[s], strategy) + 1
                - _cmp(fgt[s], feq[s], strategy) - _cmp(fgt[o], feq[o], strategy))
    raise ValueError("Invalid argument value for corruption side passed for evaluation")


def _ev_start(stats):
    if stats is None:
        return None
    e0 = torch.cuda.Event(enable_timing=True)
    e0.record()
    return e0


def _ev_stop(stats, e0):
    if stats is None:
        return
    e1 = torch.cuda.Event(enable_timing=True)
    e1.record()
    stats.setdefault("_events", []).append((e0, e1))


def _ev_collect(stats):
    if stats is None:
        return
    torch.cuda.synchronize()
    evs = stats.pop("_events", [])
    stats["count_ms"] = stats.get("count_ms", 0.0) + sum(a.elapsed_time(b) for a, b in evs)
    stats["count_launches"] = stats.get("count_launches", 0) + len(evs)


# ------------------------------------------------------------------------------------------------
# precision 2: exact ranks at MFMA speed (bf16 prefilter + exact re-scoring of the undecided candidates)
# ------------------------------------------------------------------------------------------------
_U32 = 2.0 ** -24   # unit roundoff of fp32


def table_norm_bounds(ent, ent_f16, k_int):
    """(max ||e||, max ||e~||, max ||e~ - e||) over the rows of the fp32 table and of its half copy, float64 on the
    device (emg_eval_prefilter_bounds) — computed from the tensors as they are NOW (a stale copy only widens the
    band, it never breaks it)."""
    return D.eval_prefilter_bounds(ent, ent_f16, k_int)


def prefilter_band(Q, Qb, k_int, bounds):
    """Per query row r, a RIGOROUS bound on |a - s| for every candidate e, where
        a = fp32-accumulated MFMA product of the half-ROUNDED operands  (what emg_eval_prefilter_f16 compares),
        s = the exact path's k-ordered fp32 fmaf chain of the fp32 operands (what decides the reference rank).
    With q~ = q + dq, e~ = e + de:   sum q~e~ - sum qe = dq.e~ + q.de,  so by Cauchy-Schwarz
        |a - s| <= ||dq|| ||e~|| + ||q|| ||de||  +  g (||q~|| ||e~|| + ||q|| ||e||),
    g = 2 (k + 32) 2^-24 bounding the accumulation error of either sum (standard gamma_k, doubled).  The norms of the
    residuals are the ACTUAL ones of this query tile / this table, not worst-case roundoff: ~0.4 x 2^-11 relative.
    Evaluated in float64 by emg_eval_prefilter_band (csrc/emg_rank.hip), inflated by 1e-6 and rounded up to float."""
    return D.eval_prefilter_band(Q, Qb, k_int, bounds)


def prefilter_band_reference(Q, Qb, k_int, bounds):
    """the same bound with torch float64 operations (tests compare the kernel against it)"""
    e_max, eb_max, de_max = (float(x) for x in bounds)
    q = Q[:, :k_int].double()
    qb = Qb[:, :k_int].double()
    nq, nqb, ndq = q.norm(dim=1), qb.norm(dim=1), (qb - q).norm(dim=1)
    g = 2.0 * (k_int + 32) * _U32
    return (ndq * eb_max + nq * de_max + g * (nqb * eb_max + nq * e_max)) * (1.0 + 1e-6)


# A table whose candidates the half-precision band cannot decide (a freshly initialised model, the first epochs of a fit: the
# scores crowd around the positive's) overflows the pair buffer in every tile: the prefilter pass is wasted and the exact kernel
# runs anyway (72 instead of 55 ms per 8192 x 1M pass).  So precision 2 asks first: ONE workgroup's worth of the call's query
# rows (128 triples) through the prefilter alone, the undecided fraction read back (~0.3 ms, remembered on the PrefilterTables
# of the evaluation run).  Above the fraction the pair buffer holds with room to spare the whole call takes the exact kernel.
_PROBE_TRIPLES = 128
_PROBE_MAX_UNDECIDED = 0.011   # (a wave's segment of the pair buffer holds 1.56 % of its 32 x 4096 candidates)


class _ExactFastForm:
    """One prefilter form of the exact-fast mode: the tables it derives, and the per-tile code of its prefilter, which
    rank_triples_device and _probe drive the same way for every form — ``prepare`` (outside the timed bracket) makes the tile's
    operands and returns (segments of the pair buffer, launch); ``launch(cnt, pairs, pcount, ties)`` starts the prefilter and
    says whether it covered the tile (False: the exact kernel does this tile)."""
    cap_factor = 1           # pair room per wave, in units of EMG_PAIR_CAP
    rows = 0                 # query rows per segment the re-scoring may rely on (32: the MFMA forms; else 0)
    probe_max = None         # the probe's undecided fraction above which the whole call takes the exact kernel (None: no probe)
    probe_min_rows = 0       # query rows the probe needs more than (else it reports 0.0: the tiles decide one by one)
    ties_form = False        # a second form of the prefilter that proves ties too (chosen by the probe)
    through_link = False     # ranks through a non-linear link too: the probe's verdict is remembered per link
    ok = True                # False: the tables are outside the form's range, the exact kernel ranks the call
    waves = 4                # waves per workgroup of the prefilter: the re-scoring's segments_per_block

    def bounds(self, e0, n):
        """what the form needs of the candidate slab [e0, e0 + n): made once, before the first tile"""
        return None


class PrefilterTables(_ExactFastForm):
    """what precision 2 derives from the entity table, built once per evaluation run (like the FilterIndex): the
    half-precision copy and the norm bounds of prefilter_band.  Valid while the table does not change.

    ``precision=2`` for DistMult/ComplEx/HolE/SimplE: a half-precision MFMA kernel decides every candidate whose score is farther
    from the positive's than a rigorous per-row error bound (prefilter_band), the others — typically 0.1-3 % — are re-scored with
    the exact f32 chain; shapes the prefilter kernel does not cover, and query tiles with too many undecided candidates, take the
    exact kernel (stats['fallback']).  Under a ``link``: per-row thresholds by bisection over the floats, proven ties where the
    link saturates (DESIGN.md 4.2 "Ranking through a link")."""
    rows, probe_max, ties_form, through_link = 32, _PROBE_MAX_UNDECIDED, True, True
    probe_min_rows = 128   # (the register-stationary kernel wants more than 128 rows: such calls take the exact kernel tile by tile)

    def __init__(self, ent, k_int):
        self.ent_f16 = D.to_f16(ent, k_int, ld_dst=D.prefilter_ld(k_int))
        self.k_int, self.waves = k_int, D.prefilter_waves(k_int)
        self._bounds = {}
        self._ent = ent
        self.undecided = {}   # (slab, side, link) -> undecided fraction a probe of the run's query rows found (_probe)

    def bounds(self, e0, n):
        if (e0, n) not in self._bounds:
            self._bounds[(e0, n)] = table_norm_bounds(self._ent[e0:e0 + n], self.ent_f16[e0:e0 + n], self.k_int)
        return self._bounds[(e0, n)]

    def prepare(self, model_id, Q, pos_int, e0, n, scale, link):
        k = self.k_int
        Qb = D.to_f16(Q, k, ld_dst=D.prefilter_ld(k))
        band = prefilter_band(Q, Qb, k, self.bounds(e0, n))
        tab = self.ent_f16[e0:e0 + n]

        def launch(cnt, pairs, pcount, ties):
            try:
                if link != L.LINK_LINEAR:   # thresholds of the linked comparison integer: bisection per row on the device
                    thr, thr4, _ = D.eval_link_thresholds(link, pos_int, band, _acc_scale(model_id, scale))
                    if ties:
                        D.eval_prefilter_f16_thr4(Qb, thr4, tab, e0, k, cnt[0], cnt[1], pairs, pcount)
                    else:
                        D.eval_prefilter_f16_thr(Qb, thr, tab, e0, k, cnt[0], pairs, pcount)
                else:
                    D.eval_prefilter_f16(model_id, Qb, pos_int, band, tab, e0, k, scale, cnt[0], pairs, pcount,
                                         cnt_eq=cnt[1] if ties else None)
            except L.EmgError:      # shape outside the register-stationary kernel (ties: segments that do not hold the bitmap)
                return False
            return True
        return D.eval_prefilter_segments(Q.shape[0], n, k), launch


class L2Tables(_ExactFastForm):
    """what the TransE-L2 exact-fast mode derives from the entity table, built once per evaluation run: the half rows
    [e | n_hi | n_lo] of the augmented contraction, the residual of the norm split and the norm bounds of the band.

    ``precision=2`` with TransE-L2: ||q-e||^2 = |q|^2 - (2q.e - |e|^2) is a contraction over k+2 coordinates and goes through the
    half-precision MFMA prefilter with thresholds derived for the squared distance, at the widths that kernel covers."""
    rows = 32

    def __init__(self, ent, k_int):
        self.ent_f16, self._res = D.to_f16_l2(ent, k_int, False)
        self.k_int, self.waves = k_int, D.prefilter_waves(k_int + 2)
        self._bounds = {}
        self._ent = ent

    def bounds(self, e0, n):
        if (e0, n) not in self._bounds:
            b3 = D.eval_prefilter_bounds(self._ent[e0:e0 + n], self.ent_f16[e0:e0 + n], self.k_int)
            self._bounds[(e0, n)] = torch.cat([b3, self._res])
        return self._bounds[(e0, n)]

    def prepare(self, model_id, Q, pos_int, e0, n, scale, link):
        k, bounds = self.k_int, self.bounds(e0, n)
        Qh, Q2 = D.to_f16_l2(Q, k, True)
        band = D.eval_prefilter_band(Q2, Qh, k, bounds[:3])
        thr = D.eval_l2_thresholds(Q, pos_int, band, bounds, k)
        tab = self.ent_f16[e0:e0 + n]

        def launch(cnt, pairs, pcount, ties):
            try:
                D.eval_prefilter_f16_thr(Qh, thr, tab, e0, k + 2, cnt[0], pairs, pcount)
            except L.EmgError:      # shape outside the register-stationary kernel: the exact kernel does this tile
                return False
            return True
        return D.eval_prefilter_segments(Q.shape[0], n, k + 2), launch


class SadTables(_ExactFastForm):
    """what the TransE-L1 exact-fast mode derives from the tables, built once per evaluation run: the range of the
    fixed-point map and the 16-bit image of the entity table.  Valid while the tables do not change.

    ``precision=2`` with TransE-L1: the same contract as PrefilterTables through a different prefilter — sums of absolute
    differences of 16-bit fixed-point images of the rows (``v_sad_u16``, csrc/emg_rank_sad.hip) bound every candidate's score
    from both sides; the undecided ones are re-scored with the exact chain."""

    def __init__(self, ent, rel, k_int):
        self.range = D.eval_sad_range(ent, rel, k_int)
        self.ent_u16 = D.eval_sad_quantize(ent, k_int, self.range)
        self.k_int = k_int

    def prepare(self, model_id, Q, pos_int, e0, n, scale, link):
        Qu = D.eval_sad_quantize(Q, self.k_int, self.range)
        thr = D.eval_sad_thresholds(pos_int, self.k_int, self.range)

        def launch(cnt, pairs, pcount, ties):
            D.eval_prefilter_sad(Qu, thr, self.ent_u16[e0:e0 + n], e0, self.k_int, cnt[0], pairs, pcount)
            return True
        return D.eval_sad_segments(Q.shape[0], n), launch


ROTATE_ENT_MAX = 16384.0   # largest |entry| of an entity table the RotatE half image takes: scaled query rows stay below 32752


def rotate_image_scale(ent_max):
    """the power of two s in [1, 2^24] with s * ent_max <= 16384 < 2 s * ent_max: exact in f32, and it lifts the table away from the
    half subnormals (the band's flush term is 2^-14 / s per component)"""
    if not 0.0 < ent_max <= ROTATE_ENT_MAX:
        return 1.0
    return float(min(2.0 ** (math.frexp(ROTATE_ENT_MAX / ent_max)[1] - 1), 2.0 ** 24))


# The RotatE exact-fast mode asks first, as precision 2 does: on a table its band cannot decide (a fresh model: every candidate ties
# with the positive) every wave runs out of pair room and the exact kernel runs after a wasted prefilter pass (1.3 x the exact call).
# A wave's segment holds 6.25 % of its 128 x 1024 candidates; above 4 % in the probe the whole call takes the exact kernel.
_ROTATE_PROBE_MAX_UNDECIDED = 0.04


class RotateTables(_ExactFastForm):
    """what the RotatE exact-fast mode derives from the tables, built once per evaluation run: the half image of the entity
    table ((re_j, im_j) adjacent, csrc/emg_rank_rotate.hip), its scale, rho_e per row, (max rho_e, max |e|, refused) on the device and the range
    verdict ``ok`` — False for a table with an entry that is not finite or above ROTATE_ENT_MAX (or a phase table the range pass
    refuses): such a table is ranked by the exact kernel.  Valid while the tables do not change.

    The mode ('auto' for RotatE): a half-precision prefilter on those images (the band and its proof: DESIGN.md 4.5 "Exact-fast
    ranking"), the undecided pairs re-scored with the exact chain, the ranks bit-equal to precision 0; ``stats['rotate_fast']``
    says whether the mode applied (False: a table outside the half range, ranked by the exact kernel),
    ``stats['probe_undecided']`` / ``stats['pairs']`` / ``stats['fallback']`` as for the other modes (a probe of 128 triples
    first: a table the band cannot decide takes the exact kernel for the whole call)."""
    # a wave's segment covers 128 rows x 1024 entities; RotatE's band leaves 1.4 % of random candidates undecided at k = 200
    # where the other prefilters leave ~0.7 %: four times their room per wave
    cap_factor, probe_max = 4, _ROTATE_PROBE_MAX_UNDECIDED

    def __init__(self, ent, rel, k_int):
        self.k_int, self.ok, self.scale, self.ent_f16, self.rho_e, self.ent_stats = k_int, False, 1.0, None, None, None
        self.undecided = {}   # (slab, side) -> undecided fraction a probe of the run's query rows found (_probe)
        rng = D.eval_rotate_image(ent, k_int, 1.0, check=True, image=False)
        if rng is None or D.eval_rotate_image(rel, k_int, 1.0, check=True, image=False) is None:
            return
        ent_max = float(rng[2][1])
        if ent_max > ROTATE_ENT_MAX:
            return
        self.scale = rotate_image_scale(ent_max)
        out = D.eval_rotate_image(ent, k_int, self.scale, check=True)
        if out is not None:
            self.ent_f16, self.rho_e, self.ent_stats = out
            self.ok = True

    def prepare(self, model_id, Q, pos_int, e0, n, scale, link):
        Qh, rho_q, q_stats = D.eval_rotate_image(Q, self.k_int, self.scale)
        thr = D.eval_rotate_thresholds(pos_int, rho_q, self.k_int, self.scale, q_stats, self.ent_stats)

        def launch(cnt, pairs, pcount, ties):
            D.eval_prefilter_rotate(Qh, thr, self.ent_f16[e0:e0 + n], e0, self.k_int, cnt[0], pairs, pcount)
            return True
        return D.eval_prefilter_rotate_segments(Q.shape[0], n), launch


# 'auto' takes the RotatE exact-fast mode where resolve_auto_precision's size conditions hold.  Measured (DESIGN.md 4.5 "Exact-fast
# ranking"): faster than the exact kernel at the benchmark shape.
ROTATE_FAST_AUTO = True


# the models whose 1-vs-all score is the contraction chain fmaf(q_c, e_c, acc) on a prebuilt query row (SimplE: HolE's scaled chain on
# its own query rows — include/emgraph_hip.h, EMG_SIMPLE): the MFMA count, the f16 prefilter and the bf16 mode apply to them
CONTRACTION_MODELS = (L.DISTMULT, L.COMPLEX, L.HOLE, L.SIMPLE)


def link_prefilter_applies(model_id, link):
    """ranking THROUGH a link (``link`` != linear): the exact-fast mode exists for the contraction models, under a link whose
    comparison integer has a committed order slack (D.link_order_w: what makes the threshold bisection valid); TransE ranks
    through a link by the exact kernel"""
    return link == L.LINK_LINEAR or (model_id in CONTRACTION_MODELS and D.link_order_w(link) > 0)


def resolve_auto_precision(model_id, k_int, n_test, n_ent, entities_subset=None, link=L.LINK_LINEAR):
    """what precision 'auto' means for a call: the exact-fast mode (2) returns the SAME ranks as precision 0, bit for bit,
    and pays off once the 1-vs-all product is large enough to amortise the half-precision copy of the table; its kernels
    cover the common widths.  Under a ``link``: the contraction models only (link_prefilter_applies)."""
    if not link_prefilter_applies(model_id, link):
        return 0
    covered = lambda w: 32 < w <= D.prefilter_max_cols()   # noqa: E731  (the prefilter kernel pads a width up to its next instantiation)
    applies = ((model_id in CONTRACTION_MODELS and covered(k_int)) or (model_id == L.TRANSE_L1 and k_int >= 16)
               or (model_id == L.TRANSE_L2 and covered(k_int + 2))
               or (model_id == L.ROTATE and ROTATE_FAST_AUTO and link == L.LINK_LINEAR))   # (RotatE: reachable through 'auto' only)
    return 2 if (applies and entities_subset is None and n_test >= 128 and n_ent >= 32768) else 0


_FORMS = {L.TRANSE_L1: SadTables, L.TRANSE_L2: L2Tables, L.ROTATE: RotateTables}   # a model's exact-fast form; every other model: PrefilterTables


def derived_tables(model_id, ent, rel, k_int):
    """the tables the exact-fast mode derives from the embedding tables (half-precision copy + norm bounds, 16-bit image +
    range, augmented half rows): valid while the tables do not change — a fitted model keeps them (get_ranks)"""
    form = _FORMS.get(model_id, PrefilterTables)
    return form(ent, k_int) if form in (PrefilterTables, L2Tables) else form(ent, rel, k_int)


_pair_buffers = {}


def _pair_buffer(device, n_seg, cap_factor=1):
    """(pairs int64 [cap], per-segment counts int32 [n_seg + 1]) scratch of the prefilter, cached per device.
    A wave of the prefilter covers 32 query rows x up to 4096 entities; 2048 entries hold 1.5 % of them undecided
    (random positives on Gaussian tables leave ~0.7 %, a trained model a tenth of that) — and 2048 entries are what the
    prefilter's bitmap form needs of a segment (64 per entity tile, emg_rank_bf16.hip MODE 3; below it the slower emitting form
    runs): the buffer grows with the call, 1 GiB at 8192 query rows x 1M entities, at most 4 GiB (EMG_PAIR_LOG2 = log2 entries)."""
    per = max(64, min(cap_factor * int(_switches.get("EMG_PAIR_CAP")), (1 << int(_switches.get("EMG_PAIR_LOG2"))) // max(n_seg, 1)))
    cap = n_seg * per
    key = (device.type, device.index)
    buf = _pair_buffers.get(key)
    if buf is None or buf[0].numel() < cap or buf[1].numel() < n_seg + 1:
        buf = (torch.empty(cap, dtype=torch.int64, device=device), torch.zeros(n_seg + 1, dtype=torch.int32, device=device))
        _pair_buffers[key] = buf
    return buf[0][:cap], buf[1][:n_seg + 1]


_tile_buffers = {}


def _tile_buffers_for(device, pairs, n_local):
    """(sorted pairs int64 [pairs.numel()], tile workspace uint8) scratch of the tile-major re-scoring, cached per device; the
    workspace is zero between calls (the library leaves it so)"""
    key = (device.type, device.index)
    buf = _tile_buffers.get(key)
    need = D.rescore_tiles_ws_bytes(n_local)
    if buf is None or buf[0].numel() < pairs.numel() or buf[1].numel() < need:
        buf = (torch.empty(pairs.numel(), dtype=torch.int64, device=device), torch.zeros(need, dtype=torch.uint8, device=device))
        _tile_buffers[key] = buf
    return buf[0][:pairs.numel()], buf[1]


def _rescore(model_id, Q, pos_int, slab, e0, k_int, scale, pairs, pcount, n_seg, cnt, waves, rows, link=L.LINK_LINEAR):
    """exact re-scoring of the prefilter's undecided pairs: segment-wise with the query rows in LDS (the default), or
    entity-tile-major (EMG_RESCORE=tiles: the pairs bucketed by tile of 32 entity rows, the tile's rows in LDS, query rows
    streamed).  Measured at C4's size (round 5, profiles/r5_*_pmc_rescore.txt): the segment form already finds 88 % of its
    rows in L2 and both forms are bound by LDS instruction issue (4800 bytes through LDS per pair), so the tile form's L2
    hits buy nothing: 19.2 against 17.1 ms per 8192 query rows."""
    mode = _switches.get("EMG_RESCORE")
    if mode == "tiles" and rows == 32 and link == L.LINK_LINEAR:   # (under a link: the segment form, which carries it)
        sorted_pairs, tile_ws = _tile_buffers_for(Q.device, pairs, slab.shape[0])
        try:
            D.eval_rescore_pairs_tiles(model_id, Q, pos_int, slab, e0, k_int, scale, pairs, pcount, n_seg, sorted_pairs, tile_ws, cnt[0], cnt[1])
            return
        except L.EmgError:   # rows that are not 16-byte aligned / an image that does not fit LDS: the segment form
            pass
    D.eval_rescore_pairs(model_id, Q, pos_int, slab, e0, k_int, scale, pairs, pcount, n_seg, cnt[0], cnt[1], waves, rows, link=link)


def _acc_scale(model_id, scale):
    """score = fl(accumulator * this): what carries a score-domain threshold to the prefilter's accumulator domain"""
    return float(scale) if model_id in (L.HOLE, L.SIMPLE) else 1.0


def _probe(fast, model_id, ent, rel, e0, n_cand, scale, T, side_mode, link, ties=False):
    """the undecided fraction of the call's first 128 triples through the form's prefilter alone (1.0: a wave ran out of room)"""
    Tt = torch.from_numpy(np.ascontiguousarray(T[:_PROBE_TRIPLES])).to(ent.device)
    Q, pos_int = D.eval_build_queries(model_id, ent, rel, fast.k_int, scale, Tt, side_mode, link=link)
    n_rows = Q.shape[0]
    if n_rows <= fast.probe_min_rows or n_cand == 0:
        return 0.0
    n_seg, launch = fast.prepare(model_id, Q, pos_int, e0, n_cand, scale, link)
    pairs, pcount = _pair_buffer(ent.device, n_seg, fast.cap_factor)
    cnt = torch.zeros((2, n_rows), dtype=torch.int32, device=ent.device)
    if not launch(cnt, pairs, pcount, ties):
        return 1.0 if ties else 0.0   # (the ties form needs segments that hold the bitmap: without it, the exact kernel)
    over, n_pairs = (int(v) for v in torch.stack([pcount[n_seg].long(), pcount[:n_seg].sum()]).cpu())
    return 1.0 if over else n_pairs / float(n_rows * n_cand)


def _exact_fast_form(form, ent_f16, model_id, ent, rel, k_int, scale, e0, n_cand, T, side_mode, link, n_tiles, stats):
    """(the tables of the call's exact-fast form, whether its prefilter proves ties too) — or (None, False): the exact kernel ranks
    the whole call, because the tables are outside the form's range or the probe found the band deciding too little.
    ``ent_f16``: the run's tables when it is an instance of ``form``; anything else (None included) builds them here."""
    fast = ent_f16 if isinstance(ent_f16, form) else derived_tables(model_id, ent, rel, k_int)
    if form is RotateTables and stats is not None:
        stats["rotate_fast"] = fast.ok
    if not fast.ok:
        return None, False
    fast.bounds(e0, n_cand)
    if fast.probe_max is None or len(T) < _PROBE_TRIPLES or n_cand == 0 or _switches.get("EMG_PREFILTER_PROBE") == "0":
        return fast, False
    key = (e0, n_cand, side_mode, link) if fast.through_link else (e0, n_cand, side_mode)
    und = fast.undecided.get(key)
    if und is None:
        und = _probe(fast, model_id, ent, rel, e0, n_cand, scale, T, side_mode, link)
        if und > fast.probe_max and fast.ties_form and _switches.get("EMG_PREFILTER_TIES") != "0":
            # too many undecided candidates — on a table whose scores are small against the comparison's quantum (a fresh model,
            # the first epochs of a fit) they are TIES with the positive, which the second form of the prefilter proves as it
            # proves the other two outcomes (emg_rank_bf16.hip MODE 4): probe it too
            und_t = _probe(fast, model_id, ent, rel, e0, n_cand, scale, T, side_mode, link, ties=True)
            if und_t <= fast.probe_max:
                und = -1.0 - und_t   # (negative: "the ties form decides this table", remembered like the fraction)
        fast.undecided[key] = und
    prove_ties = und < 0.0
    if stats is not None:
        stats["probe_undecided"] = -1.0 - und if prove_ties else und
        if fast.ties_form:
            stats["prove_ties"] = prove_ties
    if und > fast.probe_max:   # the band decides too little here: every tile of the call by the exact kernel
        if stats is not None:
            stats["fallback"] = stats.get("fallback", 0) + n_tiles
        return None, False
    return fast, prove_ties


def check_typed_ranking(type_constraints, entities_subset, precision, shard, link):
    """what typed ranking refuses, before any device work (rank_triples_device's docstring says why)"""
    from ..type_constraints import TypeConstraints
    if not isinstance(type_constraints, TypeConstraints):
        raise ValueError("type_constraints must be a TypeConstraints (emgraph_amd.evaluation), got {!r}".format(type(type_constraints)))
    if entities_subset is not None:
        raise ValueError("type_constraints and entities_subset (corruption_entities) both name the candidates: pass one of them")
    if link != L.LINK_LINEAR:
        raise NotImplementedError("typed ranking through a non-linear link (rank_through_link) is not available")
    if shard is not None and shard[1] > 1:
        raise NotImplementedError("typed ranking runs on one GPU: sharded evaluation is not available")
    if precision == 1:
        raise NotImplementedError("typed ranking is exact: the bf16 throughput mode (precision 1) has no typed form")
    if precision not in (0, 2, "auto"):
        raise ValueError("precision must be 0 (exact f32), 1 (bf16 MFMA), 2 (exact via half-precision prefilter) or 'auto' (0 or 2)")


_LIST_SIDES = {"s": ("s",), "o": ("o",), "s+o": ("o", "s"), "s,o": ("o", "s")}   # in the row order of emg_eval_build_queries


def check_list_ranking(candidates, corrupt_side, n_test, entities_subset, type_constraints, precision, shard, link):
    """what ranking against per-triple candidate lists refuses, before any device work (rank_triples_device's docstring says why);
    returns the normalised ``candidates``: an int K, or {'s' / 'o': int32 [n_test, K]} for the sides ``corrupt_side`` uses"""
    if entities_subset is not None:
        raise ValueError("candidates and entities_subset (corruption_entities) both name the candidates: pass one of them")
    if type_constraints is not None:
        raise ValueError("candidates and type_constraints both name the candidates: pass one of them")
    if corrupt_side not in _LIST_SIDES:
        raise ValueError("Invalid argument value for corruption side passed for evaluation")
    if link != L.LINK_LINEAR:
        raise NotImplementedError("ranking against candidate lists through a non-linear link (rank_through_link) is not available")
    if shard is not None and shard[1] > 1:
        raise NotImplementedError("ranking against candidate lists runs on one GPU: sharded evaluation is not available")
    if precision == 1:
        raise NotImplementedError("ranking against candidate lists is exact: the bf16 throughput mode (precision 1) has no such form")
    if precision not in (0, 2, "auto"):
        raise ValueError("precision must be 0 (exact f32), 1 (bf16 MFMA), 2 (exact via half-precision prefilter) or 'auto' (0 or 2)")
    if isinstance(candidates, (int, np.integer)) and not isinstance(candidates, bool):
        if candidates < 1:
            raise ValueError("candidates must be at least 1, got %d" % candidates)
        if candidates >= (1 << 31):
            raise ValueError("candidates must fit 31 bits")
        return int(candidates)
    if not isinstance(candidates, dict):
        raise ValueError("candidates must be None, an int K or a dict with int arrays [n, K] under 's' and / or 'o', got {!r}"
                         .format(type(candidates)))
    out, width = {}, None
    for side in _LIST_SIDES[corrupt_side]:
        if side not in candidates:
            raise ValueError("candidates has no list for side '%s', which corrupt_side='%s' ranks" % (side, corrupt_side))
        a = np.asarray(candidates[side])
        if a.ndim != 2 or a.shape[0] != n_test or not np.issubdtype(a.dtype, np.integer):
            raise ValueError("candidates['%s'] must be an integer array [%d, K], got %s %r" % (side, n_test, a.dtype, a.shape))
        if a.shape[1] < 1:
            raise ValueError("candidates['%s'] holds no candidate (K < 1)" % side)
        if width is not None and a.shape[1] != width:
            raise ValueError("the lists of the two sides must have the same width (pad the shorter with -1)")
        width = a.shape[1]
        if a.dtype != np.int32:   # an id beyond int32 is no entity: padding
            a = np.where((a >= 0) & (a < (1 << 31)), a, -1).astype(np.int32)
        out[side] = np.ascontiguousarray(a)
    return out


class RankMode(typing.NamedTuple):
    """what resolve_rank_mode decides for a call of rank_triples_device"""
    path: str                       # 'lists' | 'typed' | 'exact' | 'bf16' | 'exact_fast'
    form: type = None               # exact_fast: the tables class that owns the prefilter form (PrefilterTables, L2Tables, SadTables, RotateTables)
    link_exact_only: bool = False   # ranked through a link for which only the exact kernel exists (stats['link_exact_only'])
    candidates: object = None       # lists: the normalised ``candidates`` (check_list_ranking)


def _check_link(link):
    if link not in L.LINK_IDS.values():
        raise ValueError("link must be one of the L.LINK_* ids, got {!r}".format(link))


def _check_side_strategy(corrupt_side, strategy):
    if corrupt_side not in L.EVAL_SIDE_IDS:
        raise ValueError("Invalid argument value for corruption side passed for evaluation")
    if strategy not in ("worst", "best", "middle"):
        raise AssertionError("Invalid score comparision type!")


def resolve_rank_mode(model_id, k_int, n_test, n_ent, precision=0, link=L.LINK_LINEAR, shard=None, entities_subset=None,
                      type_constraints=None, candidates=None, corrupt_side="s,o", strategy="worst"):
    """The path a call of rank_triples_device takes, and every refusal that does not need the tables: a RankMode.  Pure host
    code (no tensor, no launch): the model asks it too, to know whether the derived tables are wanted (get_ranks_idx).  The order
    of the rules is the order of the refusals."""
    _check_link(link)
    sharded = shard is not None and shard[1] > 1
    if candidates is not None:
        candidates = check_list_ranking(candidates, corrupt_side, n_test, entities_subset, type_constraints, precision, shard, link)
        _check_side_strategy(corrupt_side, strategy)
        return RankMode("lists", candidates=candidates)
    if type_constraints is not None:
        check_typed_ranking(type_constraints, entities_subset, precision, shard, link)
        _check_side_strategy(corrupt_side, strategy)
        return RankMode("typed")
    rot = False   # RotatE exact-fast mode: what 'auto' resolves to for RotatE (an explicit precision 2 stays refused below)
    if precision == "auto":
        precision = resolve_auto_precision(model_id, k_int, n_test, n_ent, entities_subset, link)
        if model_id == L.ROTATE:
            rot, precision = precision == 2 and not sharded, 0
    link_exact_only = False
    if link != L.LINK_LINEAR:
        if precision == 1:
            raise NotImplementedError("the bf16 throughput mode (precision 1) does not rank through a non-linear link")
        if not link_prefilter_applies(model_id, link):
            if precision == 2:
                precision = 0   # TransE under a link (or a link without an order slack): the exact kernel, same ranks
            link_exact_only = True
    if model_id == L.TRANSE_P:
        precision = 0   # TransE with an order of the norm other than 1 / 2: the exact chain kernel (same ranks, no prefilter form)
    if model_id == L.ROTATE:
        if precision in (1, 2):
            raise NotImplementedError("RotatE is ranked by the exact kernel (precision 0 or 'auto'): precision {} has no RotatE "
                                      "form".format(precision))
        if sharded:
            raise NotImplementedError("RotatE is ranked on one GPU: sharded evaluation is not available")
    if model_id == L.SIMPLE and sharded:
        raise NotImplementedError("SimplE is ranked on one GPU: sharded evaluation is not available")
    if precision not in (0, 1, 2):
        raise ValueError("precision must be 0 (exact f32), 1 (bf16 MFMA), 2 (exact via half-precision prefilter) or 'auto' (0 or 2)")
    if precision == 2 and entities_subset is not None:
        precision = 0   # candidate lists go through the exact kernel: same ranks
    if precision == 1 and model_id not in CONTRACTION_MODELS:
        raise ValueError("the bf16 MFMA mode needs a contraction model (DistMult, ComplEx, HolE, SimplE)")
    _check_side_strategy(corrupt_side, strategy)
    if rot or precision == 2:   # (TransE-L1: the fixed-point prefilter; TransE-L2: the MFMA prefilter on the augmented rows)
        return RankMode("exact_fast", _FORMS.get(model_id, PrefilterTables), link_exact_only)
    return RankMode("bf16" if precision == 1 else "exact", None, link_exact_only)


def _filter_index(filter_triples):
    """``filter_triples`` (None, int triples or a FilterIndex) as a FilterIndex, or None"""
    if filter_triples is None or isinstance(filter_triples, FilterIndex):
        return filter_triples
    return FilterIndex(filter_triples)


def _upload_csr(ptr, idx, device, non_blocking=False):
    return torch.from_numpy(ptr).to(device, non_blocking=non_blocking), torch.from_numpy(idx).to(device, non_blocking=non_blocking)


def _assemble_ranks(chunks, corrupt_side, strategy, stats):
    """the end of a ranking call: per chunk (counters int32 [2 or 4, n_rows] on the device, its triples, single) ONE D2H and
    ranks_from_counts — two rows of counters: no filter counters; ``single``: row 0 already is what the strategy reads"""
    out = []
    for cnt, nq, single in chunks:
        c = cnt.cpu().numpy().astype(np.int64)
        if single:
            c[1] = 0
        fgt, feq = (c[2], c[3]) if len(c) == 4 else (0 * c[0], 0 * c[1])
        out.append(ranks_from_counts(c[0], c[1], fgt, feq, nq, corrupt_side, strategy))
    _ev_collect(stats)
    if not out:
        return np.zeros((0, 2) if corrupt_side == "s,o" else (0,), dtype=np.int64)
    return np.concatenate(out, axis=0)


def _rank_typed(model_id, ent, rel, k_int, scale, T, side_mode, findex, corrupt_side, strategy, query_chunk, tc, stats):
    """TYPED ranks (``type_constraints`` = ``tc``, a TypeConstraints) — (s, p, ?) is ranked among the range pool of p, (?, p, o)
    among its domain pool, a side without a constraint among all entities.  For each triple and side the rank is what
    ``rank_triples_device(that triple, corrupt_side=<side>, entities_subset=<pool>, precision=0)`` returns — a true entity outside
    its pool is treated as that call treats it: it is not a candidate and not in the filter set — with every pool of a query
    chunk counted by ONE launch (emg_eval_count_grouped, csrc/emg_rank_typed.hip).  A filter entry counts only if it lies in the
    row's pool; 's+o' adds the two sides' counters as it does untyped.  ``precision`` 'auto', 0 and 2 give the same exact ranks
    through that kernel; an explicit 1, a non-linear ``link`` and a ``shard`` of more than one rank raise NotImplementedError,
    ``entities_subset`` beside it a ValueError (check_typed_ranking).  ``stats['typed_groups']``: the pools met,
    ``stats['typed_pairs']``: sum of rows x |pool| over the typed rows.

    The triples are stably sorted by relation (the rows of a group become consecutive), per chunk ONE emg_eval_count_grouped over
    the rows that have a pool and ONE emg_eval_count over the rows that have none (all entities), the filter CSR cut down to the
    pools, the ranks put back in the caller's order."""
    from ..type_constraints import DOMAIN, RANGE
    n, n_ent = T.shape[0], int(ent.shape[0])
    if tc.n_ent != n_ent or tc.n_rel != int(rel.shape[0]):
        raise ValueError("type_constraints were built for %d entities and %d relations, the tables hold %d and %d"
                         % (tc.n_ent, tc.n_rel, n_ent, int(rel.shape[0])))
    order = np.argsort(T[:, 1], kind="stable")
    Ts = np.ascontiguousarray(T[order])
    pool_ptr, pool_idx = tc.device(ent.device)
    sizes = tc.sizes()
    pending, groups_met, pairs = [], set(), 0
    for c0 in range(0, n, query_chunk):
        Tc = Ts[c0:c0 + query_chunk]
        nq = Tc.shape[0]
        Tt = torch.from_numpy(Tc).to(ent.device)
        Q, pos_int = D.eval_build_queries(model_id, ent, rel, k_int, scale, Tt, side_mode)
        n_rows = Q.shape[0]
        p = Tc[:, 1].astype(np.int64)
        parts = []   # in the row order of emg_eval_build_queries: object-side rows first
        if side_mode in (L.EVAL_O, L.EVAL_SPO, L.EVAL_S_O):
            parts.append(tc.row_groups(p, RANGE))
        if side_mode in (L.EVAL_S, L.EVAL_SPO, L.EVAL_S_O):
            parts.append(tc.row_groups(p, DOMAIN))
        rg = np.concatenate(parts)
        typed = rg >= 0
        cnt = torch.zeros((4, n_rows), dtype=torch.int32, device=ent.device)
        ev = _ev_start(stats)
        if typed.any():
            D.eval_count_grouped(model_id, Q, pos_int, torch.from_numpy(rg.astype(np.int32)).to(ent.device), ent, k_int, scale,
                                 pool_ptr, pool_idx, cnt[0], cnt[1])
        if typed.all():
            pass
        elif not typed.any():
            D.eval_count(model_id, Q, pos_int, ent, k_int, scale, cnt[0], cnt[1])
        else:   # emg_eval_count has no per-row mask: the rows without a pool, compacted, against the whole table
            rows = torch.from_numpy(np.flatnonzero(~typed)).to(ent.device)
            sub = torch.zeros((2, rows.numel()), dtype=torch.int32, device=ent.device)
            D.eval_count(model_id, Q.index_select(0, rows), pos_int.index_select(0, rows), ent, k_int, scale, sub[0], sub[1])
            cnt[0:2].index_copy_(1, rows, sub)
        _ev_stop(stats, ev)
        if findex is not None:   # (built on the host underneath the count kernels)
            ptr, idx = tc.intersect_filter(*findex.csr(Tc, side_mode, n_ent), rg)
            D.eval_filter_count(model_id, Q, pos_int, ent, 0, k_int, scale, *_upload_csr(ptr, idx, ent.device, non_blocking=True),
                                cnt[2], cnt[3])
        groups_met.update(np.unique(rg[typed]).tolist())
        pairs += int(sizes[rg[typed]].sum())
        pending.append((cnt, nq, False))
    if stats is not None:
        stats["typed_groups"] = stats.get("typed_groups", 0) + len(groups_met)
        stats["typed_pairs"] = stats.get("typed_pairs", 0) + pairs
    sorted_ranks = _assemble_ranks(pending, corrupt_side, strategy, stats)
    ranks = np.empty_like(sorted_ranks)
    ranks[order] = sorted_ranks
    return ranks


def _rank_lists(model_id, ent, rel, k_int, scale, T, side_mode, findex, corrupt_side, strategy, query_chunk, candidates,
                candidates_seed, stats):
    """SAMPLED ranks — every triple is ranked against a candidate list of its OWN (OGB's head_neg / tail_neg, DGL-KE's
    neg_sample_size_eval, PyKEEN's SampledRankBasedEvaluator).  ``candidates`` (as check_list_ranking returns it): a dict holds int
    arrays [n, K] under 's' (subject-side lists) and / or 'o' (object-side lists), row i for test triple i, every side
    ``corrupt_side`` uses present (else ValueError); an id outside [0, n_ent) is padding (ragged lists are padded with -1).  An int
    K draws K ids per triple and side on the device, uniformly with replacement (emg_eval_draw_candidates: Philox keyed by
    ``candidates_seed``, the triple's position in ``test_triples``, the side and the column — the lists do not depend on
    ``query_chunk``).  The rank of a triple on a side is 1 + ``_cmp`` over the entries of its list that are not excluded.  With
    ``filter_triples`` the excluded entries are the row's filter set, its own true entity included; without a filter nothing is
    excluded, and a true entity that occurs in its list ties with itself, as in unfiltered ranking elsewhere.  A duplicate counts
    each time it occurs.  's+o' adds the two sides' counters as untyped ranking does.  For a list of distinct in-range ids the rank
    equals ``rank_triples_device(that triple alone, corrupt_side=<side>, entities_subset=<its list>, precision=0)`` (one exception,
    under 'middle' with a filter: that call rounds the list's ties and the filtered ties separately, this path the surviving ties
    once — they differ by one when an excluded entry and a surviving one both tie with the positive).  Per chunk
    ONE launch (emg_eval_count_lists, csrc/emg_rank_lists.hip) counts and excludes; ``precision`` 0, 2 and 'auto' all take that
    exact kernel.  ``candidates`` beside ``entities_subset`` or ``type_constraints``, a side missing, K < 1: ValueError; a
    non-linear ``link``, a ``shard`` of more than one rank, ``precision`` 1: NotImplementedError — all before any device work
    (check_list_ranking).  ``stats['list_pairs']``: rows x K; ``count_ms`` as for the other paths.  Per chunk: the query rows, the
    chunk's lists (uploaded, or drawn), the filter CSR as the exclusion, that one launch; no filter counters."""
    n, n_ent = T.shape[0], int(ent.shape[0])
    pending, pairs = [], 0
    for c0 in range(0, n, query_chunk):
        Tc = T[c0:c0 + query_chunk]
        nq = Tc.shape[0]
        Tt = torch.from_numpy(Tc).to(ent.device)
        Q, pos_int = D.eval_build_queries(model_id, ent, rel, k_int, scale, Tt, side_mode)
        n_rows = Q.shape[0]
        if isinstance(candidates, dict):
            lists = np.concatenate([candidates[side][c0:c0 + nq] for side in _LIST_SIDES[corrupt_side]], axis=0)
            cand = torch.from_numpy(np.ascontiguousarray(lists)).to(ent.device)
        else:   # keyed by the triple's position in the whole test set: the same lists whatever the chunk
            cand = D.eval_draw_candidates(nq, c0, side_mode, candidates, n_ent, candidates_seed, ent.device)
        xp = xi = None
        if findex is not None:
            xp, xi = _upload_csr(*findex.csr(Tc, side_mode, n_ent), ent.device)
        cnt = torch.zeros((2, n_rows), dtype=torch.int32, device=ent.device)
        ev = _ev_start(stats)
        D.eval_count_lists(model_id, Q, pos_int, ent, k_int, scale, cand, cnt[0], cnt[1], excl_ptr=xp, excl_idx=xi)
        _ev_stop(stats, ev)
        pairs += n_rows * int(cand.shape[1])
        pending.append((cnt, nq, False))
    if stats is not None:
        stats["list_pairs"] = stats.get("list_pairs", 0) + pairs
    return _assemble_ranks(pending, corrupt_side, strategy, stats)


def rank_triples_device(model_id, ent, rel, k_int, scale, test_triples, corrupt_side="s,o", strategy="worst",
                        filter_triples=None, entities_subset=None, query_chunk=4096, precision=0, shard=None,
                        ent_bf16=None, stats=None, ent_f16=None, link=L.LINK_LINEAR, type_constraints=None, candidates=None,
                        candidates_seed=0):
    """Ranks of ``test_triples`` (int ids) against all entities (or ``entities_subset``).  resolve_rank_mode decides the path
    and raises every refusal; what a path means is said where it is implemented.

    ``shard=(rank, world)`` (multi-GPU, see parallel.py): every rank holds the tables, scores the query tile
    against ITS contiguous candidate range only and the int32 counters are all-reduced (RCCL) before the
    ranks are assembled — exact, because counts are integers.

    ``precision=1``: bf16 MFMA throughput mode for DistMult/ComplEx/HolE (ranks agree with the exact f32 path
    statistically, not bit for bit); ``ent_bf16`` optionally passes a cached bf16 copy of the table.

    ``precision=2``: EXACT ranks (bit-equal to precision 0) at MFMA speed, through the prefilter form of the model:
    PrefilterTables (DistMult/ComplEx/HolE/SimplE), SadTables (TransE-L1), L2Tables (TransE-L2).  ``ent_f16``: the run's tables —
    an instance of that class (derived_tables); anything else, None and a raw half tensor included, is ignored and the tables are
    built inside this call.

    ``precision='auto'``: 2 where it applies and pays (contraction model, or TransE-L2 with k+2, at a width the prefilter kernel
    covers, or TransE-L1; no candidate list, at least 128 test triples against at least 32768 entities), else 0 — the ranks are the same either way.

    RotatE: ``precision='auto'`` under the same size conditions (linear link, no candidate list, one GPU) takes the RotatE
    exact-fast mode (RotateTables).  An explicit precision 1 or 2 stays refused (NotImplementedError), and so does sharded RotatE
    ranking.

    ``link`` (L.LINK_*; default linear): rank THROUGH the score link, as the reference does for a model trained with
    ``non_linearity`` (EmbeddingModel.py:1868-1879): the comparison integer is int32(phi(score) * 1e5), phi with the bits of the
    training step.  Precision 0 for all six models; precision 2 / 'auto' for the contraction models (PrefilterTables), TransE takes
    precision 0 (``stats['link_exact_only']``); precision 1 is not available (NotImplementedError).

    ``stats`` (dict, optional): receives ``count_ms`` = device time of the 1-vs-all count kernel launches
    (HIP events on the launch stream) and ``count_launches``.

    ``type_constraints`` (a TypeConstraints; default None: nothing changes): typed ranks, _rank_typed.

    ``candidates`` (default None: nothing changes) with ``candidates_seed``: sampled ranks, every triple against a candidate list
    of its own, _rank_lists."""
    _check_link(link)
    n_test = int(np.asarray(test_triples).reshape(-1, 3).shape[0])
    n_ent = 0 if candidates is not None or type_constraints is not None else int(ent.shape[0])   # (those refuse before the tables are looked at)
    mode = resolve_rank_mode(model_id, k_int, n_test, n_ent, precision, link, shard, entities_subset, type_constraints,
                             candidates, corrupt_side, strategy)
    if mode.link_exact_only and stats is not None:
        stats["link_exact_only"] = True
    T = np.ascontiguousarray(np.asarray(test_triples, dtype=np.int32).reshape(-1, 3))
    side_mode, findex = L.EVAL_SIDE_IDS[corrupt_side], _filter_index(filter_triples)
    if mode.path == "lists":
        return _rank_lists(model_id, ent, rel, k_int, scale, T, side_mode, findex, corrupt_side, strategy, query_chunk,
                           mode.candidates, candidates_seed, stats)
    if mode.path == "typed":
        return _rank_typed(model_id, ent, rel, k_int, scale, T, side_mode, findex, corrupt_side, strategy, query_chunk,
                           type_constraints, stats)
    bf16 = mode.path == "bf16"
    n = T.shape[0]
    rank, world = shard if shard is not None else (0, 1)
    from .. import parallel
    cand = None
    slab, e0 = ent, 0
    subset_local = entities_subset
    if entities_subset is not None:
        sub = np.ascontiguousarray(np.asarray(entities_subset, dtype=np.int32))
        if world > 1:
            r0, r1 = parallel.entity_range(len(sub), rank, world)
            sub = sub[r0:r1]
        subset_local = sub
        cand = torch.from_numpy(sub).to(ent.device)
    elif world > 1:
        e0, e1 = parallel.entity_range(n_ent, rank, world)
        slab = ent[e0:e1]
    n_slab = slab.shape[0]
    fast, prove_ties = None, False   # the exact-fast form of the call (its tables) and whether its prefilter proves ties too
    if mode.path == "exact_fast":
        fast, prove_ties = _exact_fast_form(mode.form, ent_f16, model_id, ent, rel, k_int, scale, e0, n_slab, T, side_mode, link,
                                            (n + query_chunk - 1) // query_chunk, stats)
    pending = []  # (counters on the device, nq) per chunk: every launch is asynchronous, ONE D2H at the end
    for c0 in range(0, n, query_chunk):
        Tc = T[c0:c0 + query_chunk]
        nq = Tc.shape[0]
        Tt = torch.from_numpy(Tc).to(ent.device)
        Q, pos_int = D.eval_build_queries(model_id, ent, rel, k_int, scale, Tt, side_mode, link=link)
        n_rows = Q.shape[0]
        cnt = torch.zeros((4, n_rows), dtype=torch.int32, device=ent.device)
        have_cands = cand.numel() > 0 if cand is not None else n_slab > 0
        if bf16:
            # bf16 MFMA throughput mode (statistical rank agreement; see emg_rank_bf16.hip)
            kp = D.bf16_ld(k_int)
            if ent_bf16 is None:
                ent_bf16 = D.to_bf16(ent, k_int, ld_dst=kp)
            Qb = D.to_bf16(Q, k_int, ld_dst=kp)
            # the true entity ties with itself by construction: pos_int comes from the same MFMA arithmetic
            pos_int, self_ent = D.eval_pos_int_bf16(model_id, ent_bf16, k_int, scale, Tt, side_mode, Qb)
            tab, off = (ent_bf16, 0) if cand is not None else (ent_bf16[e0:e0 + n_slab], e0)
            # 'worst' reads only #(>=), 'best' only #(>): one comparison per score in the kernel's epilogue
            need = {"worst": 1, "best": 2, "middle": 0}[strategy]
            count = lambda: D.eval_count_bf16(model_id, Qb, pos_int, self_ent, tab, k_int, scale, cnt[0], cnt[1],  # noqa: E731
                                              cand=cand, ent_offset=off, need=need)
            fcount = lambda fp_, fi_: D.eval_filter_count_bf16(model_id, Qb, pos_int, self_ent, tab, off, k_int,  # noqa: E731
                                                               scale, fp_, fi_, cnt[2], cnt[3])
        else:
            tab, off = (ent, 0) if cand is not None else (slab, e0)
            count = lambda Q=Q, pos_int=pos_int, cnt=cnt, tab=tab: D.eval_count(  # noqa: E731  (bound now: re-run at the end on overflow)
                model_id, Q, pos_int, tab, k_int, scale, cnt[0], cnt[1], cand=cand, link=link)
            fcount = lambda fp_, fi_: D.eval_filter_count(model_id, Q, pos_int, tab, off, k_int, scale, fp_, fi_,  # noqa: E731
                                                          cnt[2], cnt[3], link=link)
        pre = None    # (overflow flag, undecided pairs) of this tile on the device + what an exact re-run needs
        if fast is not None and have_cands:
            # the form's prefilter, then exact re-scoring of the undecided pairs: both asynchronous; whether a wave ran out of
            # pair room (-> this tile is redone by the exact kernel) is read with the counters at the end
            n_seg, launch = fast.prepare(model_id, Q, pos_int, e0, n_slab, scale, link)
            pairs, pcount = _pair_buffer(ent.device, n_seg, fast.cap_factor)
            ev = _ev_start(stats)
            if launch(cnt, pairs, pcount, prove_ties):   # (False: a shape the prefilter does not cover, the exact kernel does this tile)
                _rescore(model_id, Q, pos_int, slab, e0, k_int, scale, pairs, pcount, n_seg, cnt, fast.waves, fast.rows, link=link)
                _ev_stop(stats, ev)
                pre = (torch.stack([pcount[n_seg].long(), pcount[:n_seg].sum()]), count)
        if have_cands and pre is None:
            ev = _ev_start(stats)
            count()  # the big kernel goes first: the host-side filter CSR below is built underneath it
            _ev_stop(stats, ev)
        if findex is not None:
            ptr, idx = findex.csr(Tc, side_mode, n_ent, subset_local)
            if have_cands:
                fcount(*_upload_csr(ptr, idx, ent.device, non_blocking=True))
        pending.append((cnt, nq, bf16 and strategy != "middle", pre))   # (single-counter mode: see `need` above)

    def finished():   # what a chunk's counters still need, just before their D2H
        for cnt, nq, single, pre in pending:
            if pre is not None:
                over, n_pairs = (int(v) for v in pre[0].cpu())
                if stats is not None:
                    stats["pairs"] = stats.get("pairs", 0) + (0 if over else n_pairs)
                    stats["fallback"] = stats.get("fallback", 0) + int(bool(over))
                if over:   # too many undecided candidates for the pair buffer: this tile again, by the exact kernel
                    cnt[0:2].zero_()
                    pre[1]()
            if world > 1:
                # range-sharded evaluation: the counters of this rank's candidate range are exact now (an overflowing tile has
                # been redone locally — a rank whose range did not overflow has nothing to redo), so the sum over the ranks is
                # taken HERE, after the overflow check: every rank issues the same collectives in the same order whatever
                # its own flags said (a fresh Glorot table leaves every candidate undecided: overflow is a normal state)
                parallel.allreduce_sum_(cnt)
            yield cnt, nq, single
    return _assemble_ranks(finished(), corrupt_side, strategy, stats)


def check_top_n(top_n):
    """1 <= top_n <= EMG_TOPN_MAX, as the library checks it (here: before any device work)"""
    if isinstance(top_n, bool) or not isinstance(top_n, (int, np.integer)) or not 1 <= int(top_n) <= L.TOPN_MAX:
        raise ValueError("top_n must be an integer in [1, %d] (EMG_TOPN_MAX), got %r" % (L.TOPN_MAX, top_n))
    return int(top_n)


def topn_device(model_id, ent, rel, k_int, scale, queries, side, top_n, filter_triples=None, entities_subset=None,
                query_chunk=4096, ent_chunk=0):
    """Top-N completions of ``queries`` (int ids [n, 2]: (s, p) for side 'o', (p, o) for side 's') among all entities (or
    ``entities_subset``), known completions of ``filter_triples`` excluded: (ids int32 [n, top_n], raw scores float32
    [n, top_n]), short rows padded with (-1, -inf).  Scoring and selection are one fused kernel per query tile
    (emg_eval_topn, csrc/emg_topn.hip): the [n x |E|] scores are never stored.  Every launch is asynchronous, ONE
    device-to-host copy at the end."""
    top_n = check_top_n(top_n)
    if side not in ("s", "o"):
        raise ValueError("side must be 's' or 'o'")
    q = np.asarray(queries, dtype=np.int64).reshape(-1, 2)
    n, n_ent = q.shape[0], int(ent.shape[0])
    # the unknown column holds entity 0: eval_build_queries reads it only for pos_int, which is ignored here
    T = np.zeros((n, 3), np.int32)
    if side == "o":
        T[:, 0], T[:, 1] = q[:, 0], q[:, 1]
    else:
        T[:, 1], T[:, 2] = q[:, 0], q[:, 1]
    cand, sub = None, None
    if entities_subset is not None:
        sub = np.unique(np.asarray(entities_subset, dtype=np.int64))   # de-duplicated (and ascending)
        cand = torch.from_numpy(sub.astype(np.int32)).to(ent.device)
    findex = _filter_index(filter_triples)
    n_cand = len(sub) if sub is not None else n_ent
    ws = None
    pending = []
    for c0 in range(0, n, query_chunk):
        Tt = torch.from_numpy(np.ascontiguousarray(T[c0:c0 + query_chunk])).to(ent.device)
        Q, _ = D.eval_build_queries(model_id, ent, rel, k_int, scale, Tt, L.EVAL_O if side == "o" else L.EVAL_S)
        ptr = idx = None
        if findex is not None:
            ptr, idx = _upload_csr(*findex.known_csr(q[c0:c0 + query_chunk], side, n_ent, sub), ent.device)
        if ws is None:   # one workspace for every tile: the launches are ordered on the stream (the first tile is the largest)
            ws = torch.empty(D.eval_topn_ws_bytes(Q.shape[0], n_cand, top_n, ent_chunk), dtype=torch.uint8, device=ent.device)
        pending.append(D.eval_topn(model_id, Q, ent, k_int, scale, top_n, cand=cand, excl_ptr=ptr, excl_idx=idx,
                                   ent_chunk=ent_chunk, ws=ws))
    if not pending:
        return np.zeros((0, top_n), np.int32), np.zeros((0, top_n), np.float32)
    ids = torch.cat([p[0] for p in pending]).cpu().numpy()
    scores = torch.cat([p[1] for p in pending]).cpu().numpy()
    return ids, scores


def grid_ranks_device(model_id, ent, rel, k_int, scale, rel_id, S, O, findex=None, query_chunk=4096):
    """Filtered ranks ('worst' strategy) of EVERY cell (s, rel_id, o) of the grid S x O: (rank_s, rank_o), int64 [|S|, |O|] —
    what rank_triples_device(cells, "s,o", "worst", filter_triples=findex) returns for the cells that are not in the filter,
    from |S| + |O| rows of 1-vs-all scoring instead of 2 |S| |O|.

    All cells (s, rel_id, .) share the object-side row of s, whose thresholds are the entities O; all cells (., rel_id, o)
    the subject-side row of o, with thresholds S.  A row's exclusions are its known completions (FilterIndex.known_csr), so
    a cell's rank is gt + eq of emg_eval_grid_count (csrc/emg_grid.hip): the threshold entity's own tie is the `+ 1 - self`
    of ranks_from_counts.  A cell whose triple IS in the filter is excluded from its own rows: its entries mean nothing, the
    caller masks them.  Rows go in pieces of ``query_chunk``, thresholds in pieces of EMG_GRID_THR_MAX; every launch is
    asynchronous, ONE device-to-host copy per side at the end.  One GPU."""
    S = np.asarray(S, dtype=np.int64).reshape(-1)
    O = np.asarray(O, dtype=np.int64).reshape(-1)
    n_ent = int(ent.shape[0])
    for name, ids in (("S", S), ("O", O)):
        if ids.size and not ((ids >= 0) & (ids < n_ent)).all():
            raise ValueError("%s holds an entity id outside [0, %d)" % (name, n_ent))
    if S.size == 0 or O.size == 0:
        return np.zeros((len(S), len(O)), np.int64), np.zeros((len(S), len(O)), np.int64)
    findex = _filter_index(findex)

    def side(rows, thr, side_name):
        """gt + eq [len(rows), len(thr)] of the rows (rows[i], rel_id, ?) / (?, rel_id, rows[i])"""
        T = np.zeros((len(rows), 3), np.int32)   # the unknown column holds entity 0: it only feeds pos_int, which is ignored
        T[:, 1] = rel_id
        T[:, 0 if side_name == "o" else 2] = rows
        q = np.stack([rows, np.full(len(rows), rel_id, np.int64)], 1)
        if side_name == "s":
            q = q[:, ::-1]
        thr_d = [torch.from_numpy(np.ascontiguousarray(thr[t0:t0 + L.GRID_THR_MAX], dtype=np.int32)).to(ent.device)
                 for t0 in range(0, len(thr), L.GRID_THR_MAX)]
        ws, out = None, []
        for c0 in range(0, len(rows), query_chunk):
            Tt = torch.from_numpy(np.ascontiguousarray(T[c0:c0 + query_chunk])).to(ent.device)
            Q, _ = D.eval_build_queries(model_id, ent, rel, k_int, scale, Tt, L.EVAL_O if side_name == "o" else L.EVAL_S)
            ptr = idx = None
            if findex is not None:
                ptr, idx = _upload_csr(*findex.known_csr(q[c0:c0 + query_chunk], side_name, n_ent), ent.device)
            if ws is None:   # one workspace: the launches are ordered on the stream, the first piece is the largest of each kind
                ws = torch.empty(D.eval_grid_ws_bytes(Q.shape[0], int(thr_d[0].numel())), dtype=torch.uint8, device=ent.device)
            pieces = []
            for td in thr_d:
                gt, eq = D.eval_grid_count(model_id, Q, ent, k_int, scale, td, excl_ptr=ptr, excl_idx=idx, ws=ws)
                pieces.append(gt.add_(eq))
            out.append(torch.cat(pieces, dim=1) if len(pieces) > 1 else pieces[0])
        return torch.cat(out).cpu().numpy().astype(np.int64)

    rank_o = side(S, O, "o")
    rank_s = np.ascontiguousarray(side(O, S, "s").T)
    return rank_s, rank_o


# ------------------------------------------------------------------------------------------------
# relation prediction: rank / complete (s, ?, o) against the relation table (csrc/emg_relrank.hip)
# ------------------------------------------------------------------------------------------------
def _rel_candidates(relations_subset, n_rel, device):
    """(ascending distinct ids or None, the same on the device or None)"""
    if relations_subset is None:
        return None, None
    sub = np.unique(np.asarray(relations_subset, dtype=np.int64).reshape(-1))
    if sub.size and not ((sub >= 0) & (sub < n_rel)).all():
        raise ValueError("relations_subset holds a relation id outside [0, %d)" % n_rel)
    return sub, torch.from_numpy(sub.astype(np.int32)).to(device)


def _rel_operand(model_id, rel, k_int):
    """what the relation-side kernels read as the relation table: RotatE's [cos | sin] image, made once per call"""
    return D.eval_rel_rotate_image(rel, k_int) if model_id == L.ROTATE else rel


def _check_pair_ids(name, ids, n):
    if ids.size and not ((ids >= 0) & (ids < n)).all():
        raise ValueError("%s holds an id outside [0, %d)" % (name, n))


def rank_relations_device(model_id, ent, rel, k_int, scale, test_triples, strategy="worst", filter_triples=None,
                          relations_subset=None, link=L.LINK_LINEAR, query_chunk=1 << 16, shard=None):
    """Relation-side ranks of ``test_triples`` (int ids [n, 3]): the rank of p among all relations (or ``relations_subset``)
    completing (s, ?, o), int64 [n].  A triple's score is the object side's (one triple, one score: the chain of the query row of
    (s, r) against o), the comparison is int32(score * 1e5) — through ``link`` when it is not linear — the counts run over every
    candidate, and a row's filter set is {p} U {p' : (s, p', o) in filter_triples}: ranks_from_counts(..., 'o', strategy).
    One kernel launch per ``query_chunk`` rows (emg_eval_rel_count), every launch asynchronous, ONE device-to-host copy at the
    end.  One GPU: ``shard`` with more than one rank raises NotImplementedError."""
    _check_link(link)
    if shard is not None and shard[1] > 1:
        raise NotImplementedError("relation ranking runs on one GPU: sharded evaluation is not available")
    if strategy not in ("worst", "best", "middle"):
        raise AssertionError("Invalid score comparision type!")
    T = np.ascontiguousarray(np.asarray(test_triples, dtype=np.int32).reshape(-1, 3))
    n, n_ent, n_rel = T.shape[0], int(ent.shape[0]), int(rel.shape[0])
    _check_pair_ids("test_triples (entities)", T[:, [0, 2]], n_ent)
    _check_pair_ids("test_triples (relations)", T[:, 1], n_rel)
    sub, cand = _rel_candidates(relations_subset, n_rel, ent.device)
    findex = _filter_index(filter_triples)
    rel_op = _rel_operand(model_id, rel, k_int)
    pending = []
    for c0 in range(0, n, query_chunk):
        Tc = T[c0:c0 + query_chunk]
        Tt = torch.from_numpy(Tc).to(ent.device)
        _, pos_int = D.eval_build_queries(model_id, ent, rel, k_int, scale, Tt, L.EVAL_O, link=link)
        ptr = idx = None
        if findex is not None:
            ptr, idx = _upload_csr(*findex.rel_csr(Tc, n_rel, sub), ent.device)
        pending.append(D.eval_rel_count(model_id, ent, rel_op, k_int, scale, Tt, pos_int, cand_rel=cand, excl_ptr=ptr, excl_idx=idx,
                                        link=link))
    if not pending:
        return np.zeros(0, dtype=np.int64)
    c = torch.cat(pending, dim=1).cpu().numpy().astype(np.int64)
    return ranks_from_counts(c[0], c[1], c[2], c[3], n, "o", strategy)


def topn_relations_device(model_id, ent, rel, k_int, scale, pairs, top_n, filter_triples=None, relations_subset=None,
                          query_chunk=None):
    """Top-N relations of ``pairs`` (int ids [n, 2] = (s, o)) among all relations (or ``relations_subset``), the known relations
    of a pair in ``filter_triples`` excluded: (ids int32 [n, top_n], raw scores float32 [n, top_n]), short rows padded with
    (-1, -inf), in the total order of topn_device.  Per chunk of rows the scores are written densely (the candidate table is
    small: emg_eval_rel_scores_dense) and one wave per row selects (emg_eval_rel_topn); every launch is asynchronous, ONE
    device-to-host copy at the end."""
    top_n = check_top_n(top_n)
    q = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    n, n_ent, n_rel = q.shape[0], int(ent.shape[0]), int(rel.shape[0])
    _check_pair_ids("pairs", q, n_ent)
    sub, cand = _rel_candidates(relations_subset, n_rel, ent.device)
    n_cand = len(sub) if sub is not None else n_rel
    if query_chunk is None:   # the dense chunk stays at 128 MiB
        query_chunk = max(256, min(1 << 16, (1 << 25) // max(n_cand, 1)))
    findex = _filter_index(filter_triples)
    T = np.zeros((n, 3), np.int32)   # (the kernels read s and o only)
    T[:, 0], T[:, 2] = q[:, 0], q[:, 1]
    rel_op = _rel_operand(model_id, rel, k_int)
    pending = []
    for c0 in range(0, n, query_chunk):
        Tt = torch.from_numpy(np.ascontiguousarray(T[c0:c0 + query_chunk])).to(ent.device)
        ptr = idx = None
        if findex is not None:
            ptr, idx = _upload_csr(*findex.known_rel_csr(q[c0:c0 + query_chunk], n_rel, sub), ent.device)
        S = D.eval_rel_scores_dense(model_id, ent, rel_op, k_int, scale, Tt, cand_rel=cand)
        pending.append(D.eval_rel_topn(S, top_n, cand_rel=cand, excl_ptr=ptr, excl_idx=idx))
    if not pending:
        return np.zeros((0, top_n), np.int32), np.zeros((0, top_n), np.float32)
    ids = torch.cat([p[0] for p in pending]).cpu().numpy()
    scores = torch.cat([p[1] for p in pending]).cpu().numpy()
    return ids, scores
