"""Type constraints: per relation, the entities that can be its subject (the DOMAIN pool) and its object (the RANGE pool).

Not in the reference, which ranks a triple against all entities or one global list.  The precedents are LibKGE's type-constrained
ranking and PyKEEN's pseudo-typed negatives, both built on the local closed-world assumption of Krompass et al. 2015: the pools of
a relation are the subjects / objects OBSERVED with it.  ``evaluate_performance(..., type_constraints=tc)`` and
``rank_triples_device(..., type_constraints=tc)`` rank (s, p, ?) among the range pool of p and (?, p, o) among its domain pool
(csrc/emg_rank_typed.hip: every relation's pool in one launch).

Layout: one CSR over ``2 * n_rel`` groups, group ``g = 2 * p + side``; side 0 is the domain pool (used when the SUBJECT is
corrupted), side 1 the range pool (used when the OBJECT is corrupted).  ``pool_ptr`` int64 [2 n_rel + 1], ``pool_idx`` int32:
global entity ids, ascending and distinct within a group.  A group WITHOUT a constraint is stored empty and means "all entities"
(a constraint that admits nobody cannot be stated: an explicitly empty pool is refused)."""
from __future__ import annotations

import numpy as np

DOMAIN, RANGE = 0, 1   # `side` of a group: the pool of subjects / of objects


def _sizes(model):
    if isinstance(model, (tuple, list)):
        n_ent, n_rel = (int(v) for v in model)
        return n_ent, n_rel, None, None
    return len(model.ent_to_idx), len(model.rel_to_idx), model.ent_to_idx, model.rel_to_idx


class TypeConstraints:
    """The pools of every relation (module docstring: the layout).  Build one with ``from_triples`` (the observed domains and
    ranges) or ``from_pools`` (explicit lists); the constructor takes a finished CSR and validates it."""

    def __init__(self, pool_ptr, pool_idx, n_ent, n_rel):
        n_ent, n_rel = int(n_ent), int(n_rel)
        if n_ent < 1 or n_rel < 1 or n_ent >= (1 << 31) or n_rel >= (1 << 30):
            raise ValueError("type constraints need 1 <= n_ent < 2^31 and 1 <= n_rel < 2^30")
        ptr = np.ascontiguousarray(np.asarray(pool_ptr, dtype=np.int64).reshape(-1))
        idx64 = np.asarray(pool_idx, dtype=np.int64).reshape(-1)
        if len(ptr) != 2 * n_rel + 1 or ptr[0] != 0 or ptr[-1] != len(idx64) or (np.diff(ptr) < 0).any():
            raise ValueError("pool_ptr must hold 2 * n_rel + 1 ascending offsets from 0 to len(pool_idx)")
        if idx64.size and not ((idx64 >= 0) & (idx64 < n_ent)).all():
            raise ValueError("a pool holds an entity id outside [0, %d)" % n_ent)
        group = np.repeat(np.arange(2 * n_rel, dtype=np.int64), np.diff(ptr))
        keys = group * np.int64(n_ent) + idx64
        if keys.size > 1 and not (np.diff(keys) > 0).all():
            raise ValueError("the ids of a pool must be ascending and distinct (a duplicate, or an unsorted pool)")
        self.n_ent, self.n_rel = n_ent, n_rel
        self.pool_ptr = ptr
        self.pool_idx = np.ascontiguousarray(idx64.astype(np.int32))
        self._keys = keys          # g * n_ent + e, ascending: membership of (group, entity) is one searchsorted
        self._device = {}          # (device type, index) -> (pool_ptr, pool_idx) tensors, made once

    # ---- constructors ----
    @classmethod
    def from_triples(cls, X, model, from_idx=False):
        """The observed pools: per relation the sorted distinct subjects (domain) and objects (range) of the triples ``X``
        ([n, 3] labels; ids with ``from_idx=True``, and then ``model`` may be the pair ``(n_ent, n_rel)``).  Triples with a
        label the model has not seen are dropped, as ``filter_unseen_entities`` drops them; an id out of range is a ValueError.
        A relation without triples has no constraint on either side."""
        n_ent, n_rel, ent_to_idx, rel_to_idx = _sizes(model)
        X = np.asarray(X)
        if X.ndim != 2 or X.shape[1] != 3:
            raise ValueError("X must have shape [n, 3]")
        if from_idx:
            T = X.astype(np.int64)
            if T.size and not ((T[:, [0, 2]] >= 0) & (T[:, [0, 2]] < n_ent)).all():
                raise ValueError("X holds an entity id outside [0, %d)" % n_ent)
            if T.size and not ((T[:, 1] >= 0) & (T[:, 1] < n_rel)).all():
                raise ValueError("X holds a relation id outside [0, %d)" % n_rel)
        else:
            if ent_to_idx is None:
                raise ValueError("labels need a model (its ent_to_idx / rel_to_idx); pass from_idx=True for ids")
            from .evaluation.protocol import _lookup
            (s, ok_s), (p, ok_p), (o, ok_o) = _lookup(X[:, 0], ent_to_idx), _lookup(X[:, 1], rel_to_idx), _lookup(X[:, 2], ent_to_idx)
            keep = ok_s & ok_p & ok_o
            T = np.stack([s[keep], p[keep], o[keep]], 1).astype(np.int64)
        group = np.concatenate([2 * T[:, 1] + DOMAIN, 2 * T[:, 1] + RANGE])
        keys = np.unique(group * np.int64(n_ent) + np.concatenate([T[:, 0], T[:, 2]]))
        g = keys // n_ent
        ptr = np.zeros(2 * n_rel + 1, np.int64)
        np.cumsum(np.bincount(g, minlength=2 * n_rel), out=ptr[1:])
        return cls(ptr, keys - g * n_ent, n_ent, n_rel)

    @classmethod
    def from_pools(cls, pools, model, from_idx=False):
        """Explicit pools: ``{relation: (domain, range)}`` of labels (ids with ``from_idx=True``, and then ``model`` may be the
        pair ``(n_ent, n_rel)``).  A relation that is missing, or ``None`` on one side, has no constraint there.  Every id is
        sorted into place; an unknown label or relation, an id out of range, a duplicate within a pool and an explicitly empty
        pool are ValueErrors."""
        n_ent, n_rel, ent_to_idx, rel_to_idx = _sizes(model)
        if not from_idx and ent_to_idx is None:
            raise ValueError("labels need a model (its ent_to_idx / rel_to_idx); pass from_idx=True for ids")
        per_group = {}
        for relation, sides in pools.items():
            if from_idx:
                p = int(relation)
                if not 0 <= p < n_rel:
                    raise ValueError("relation id %r outside [0, %d)" % (relation, n_rel))
            else:
                if relation not in rel_to_idx:
                    raise ValueError("unknown relation %r" % (relation,))
                p = int(rel_to_idx[relation])
            if not isinstance(sides, (tuple, list)) or len(sides) != 2:
                raise ValueError("the pools of relation %r must be a pair (domain, range)" % (relation,))
            for side, members in enumerate(sides):
                if members is None:
                    continue
                members = np.asarray(members).reshape(-1)
                if members.size == 0:
                    raise ValueError("the %s pool of relation %r is empty: pass None for 'no constraint'"
                                     % (("domain", "range")[side], relation))
                if from_idx:
                    ids = members.astype(np.int64)
                    if not ((ids >= 0) & (ids < n_ent)).all():
                        raise ValueError("the pools of relation %r hold an entity id outside [0, %d)" % (relation, n_ent))
                else:
                    from .evaluation.protocol import _lookup
                    ids, ok = _lookup(members, ent_to_idx)
                    if not ok.all():
                        raise ValueError("the pools of relation %r hold an unknown entity" % (relation,))
                ids = np.sort(ids.astype(np.int64))
                if (np.diff(ids) == 0).any():
                    raise ValueError("the %s pool of relation %r holds a duplicate" % (("domain", "range")[side], relation))
                per_group[2 * p + side] = ids
        ptr = np.zeros(2 * n_rel + 1, np.int64)
        for g, ids in per_group.items():
            ptr[g + 1] = len(ids)
        np.cumsum(ptr, out=ptr)
        idx = np.concatenate([per_group[g] for g in sorted(per_group)]) if per_group else np.zeros(0, np.int64)
        return cls(ptr, idx, n_ent, n_rel)

    # ---- what the ranking path reads ----
    @property
    def n_groups(self):
        return 2 * self.n_rel

    def sizes(self):
        """int64 [2 n_rel]: the members of every group (0: no constraint)"""
        return np.diff(self.pool_ptr)

    def pool(self, relation_id, side):
        """the ids of one pool (``side``: DOMAIN = 0 / RANGE = 1), or None where there is no constraint"""
        g = 2 * int(relation_id) + int(side)
        lo, hi = self.pool_ptr[g], self.pool_ptr[g + 1]
        return self.pool_idx[lo:hi] if hi > lo else None

    def row_groups(self, relations, side):
        """int64 group id per row for the relation ids ``relations`` on ``side``; -1 where the group has no constraint (all
        entities) or the relation id is outside [0, n_rel)"""
        p = np.asarray(relations, dtype=np.int64)
        ok = (p >= 0) & (p < self.n_rel)
        g = np.where(ok, 2 * p + int(side), 0)
        return np.where(ok & (self.sizes()[g] > 0), g, -1)

    def contains(self, groups, entities):
        """bool per (group, entity) pair: is the entity a member of the group's pool?  (False for a group < 0)"""
        g = np.asarray(groups, dtype=np.int64)
        e = np.asarray(entities, dtype=np.int64)
        ok = (g >= 0) & (e >= 0) & (e < self.n_ent)
        k = np.where(ok, g * np.int64(self.n_ent) + e, -1)
        pos = np.minimum(np.searchsorted(self._keys, k), max(len(self._keys) - 1, 0))
        return ok & (self._keys[pos] == k) if len(self._keys) else np.zeros(len(k), bool)

    def intersect_filter(self, filt_ptr, filt_idx, row_group):
        """The filter CSR of a query tile (FilterIndex.csr) with every row's entries cut down to the row's pool: a filter entry
        counts only if it is a candidate.  Rows with ``row_group`` < 0 (all entities) keep their entries."""
        filt_ptr = np.asarray(filt_ptr, dtype=np.int64)
        row_group = np.asarray(row_group, dtype=np.int64)
        rows = np.repeat(np.arange(len(row_group), dtype=np.int64), np.diff(filt_ptr))
        g = row_group[rows]
        keep = (g < 0) | self.contains(g, filt_idx)
        ptr = np.zeros(len(row_group) + 1, np.int64)
        np.cumsum(np.bincount(rows[keep], minlength=len(row_group)), out=ptr[1:])
        return ptr, np.ascontiguousarray(np.asarray(filt_idx)[keep].astype(np.int32))

    def device(self, device):
        """(pool_ptr int64, pool_idx int32) on ``device``: copied once per device and kept on the object"""
        import torch
        device = torch.device(device)
        key = (device.type, device.index)
        if key not in self._device:
            self._device[key] = (torch.from_numpy(self.pool_ptr).to(device), torch.from_numpy(self.pool_idx).to(device))
        return self._device[key]
