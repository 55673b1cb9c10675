"""Host statement of the sampled-ranking contract (include/emgraph_hip.h: emg_eval_count_lists, emg_eval_draw_candidates;
emgraph_amd/evaluation/ranking.py: rank_triples_device(candidates=...)) in numpy: the draw of the lists with the oracle's Philox,
the counters of a list walk, and the ranks of both statements of the semantics — the walk over the entries that are not excluded,
and the entities_subset rule (counters of the whole list minus the counters of its filtered members) — on a small numpy model."""
import numpy as np

from oracle.emgraph_oracle import philox4x32_10

F32 = np.float32
EVAL_S, EVAL_O, EVAL_SPO, EVAL_S_O = range(4)                     # EMG_EVAL_*
SIDES_OF = {"s": ("s",), "o": ("o",), "s+o": ("o", "s"), "s,o": ("o", "s")}   # row order of emg_eval_build_queries: object side first
SIDE_MODE = {"s": EVAL_S, "o": EVAL_O, "s+o": EVAL_SPO, "s,o": EVAL_S_O}


def cmp_int(score):
    """int32(f32(score) * f32(1e5)) in float32 arithmetic (scores far inside the int32 range)"""
    return (np.asarray(score).astype(F32) * F32(100000.0)).astype(np.int32)


# ---- the draw -----------------------------------------------------------------------------------------------------------------------
def draw_ids(g, j, sd, seed, n_ent):
    """ids of the list entries (test-set position g, column j, side bit sd: 1 = object side), broadcast over the arguments:
    o = philox4x32_10(lo32(g), hi32(g), j, sd, lo32(seed), hi32(seed));  id = (((o[2] << 32) | o[1]) * n_ent) >> 64"""
    g, j, sd = np.broadcast_arrays(np.asarray(g, dtype=np.uint64), np.asarray(j, dtype=np.uint64), np.asarray(sd, dtype=np.uint64))
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    o = philox4x32_10((g & np.uint64(0xFFFFFFFF)).astype(np.uint32), (g >> np.uint64(32)).astype(np.uint32), j.astype(np.uint32),
                      sd.astype(np.uint32), seed & 0xFFFFFFFF, seed >> 32)
    r64 = (o[2].astype(np.uint64) << np.uint64(32)) | o[1].astype(np.uint64)
    ids = (r64.astype(object) * int(n_ent)) >> 64          # exact: Python integers
    return np.asarray(ids, dtype=np.int64).astype(np.int32).reshape(g.shape)


def draw_rows(n_q, q_offset, side_mode, K, n_ent, seed):
    """int32 [n_rows, K]: what emg_eval_draw_candidates writes for n_q test triples starting at position q_offset"""
    sides = {EVAL_S: (0,), EVAL_O: (1,), EVAL_SPO: (1, 0), EVAL_S_O: (1, 0)}[side_mode]
    g = (q_offset + np.arange(n_q, dtype=np.int64))[:, None]
    j = np.arange(K, dtype=np.int64)[None, :]
    return np.concatenate([draw_ids(g, j, sd, seed, n_ent) for sd in sides], axis=0)


def draw_candidates(n_test, corrupt_side, K, n_ent, seed):
    """{'s' / 'o': int32 [n_test, K]}: the lists rank_triples_device(candidates=K, candidates_seed=seed) ranks against"""
    g = np.arange(n_test, dtype=np.int64)[:, None]
    j = np.arange(K, dtype=np.int64)[None, :]
    return {side: draw_ids(g, j, 1 if side == "o" else 0, seed, n_ent) for side in SIDES_OF[corrupt_side]}


# ---- the counters of a list walk -----------------------------------------------------------------------------------------------------
def list_counts(ci, pos_int, cand, n_cand, n_ent, excl_ptr=None, excl_idx=None):
    """(gt, eq, skipped) int64 [n_rows] from the comparison integers ci [n_rows, n_ent] of every (row, entity) pair: per row the
    entries cand[r, :n_cand] that are entities (0 <= id < n_ent) and not in the row's exclusion range, each as often as it occurs,
    that compare > / == pos_int[r]; skipped = the entries that were not counted at all"""
    n_rows = len(pos_int)
    ids = np.asarray(cand)[:, :n_cand].astype(np.int64)
    live = (ids >= 0) & (ids < n_ent)
    if excl_ptr is not None:
        keys = np.repeat(np.arange(n_rows, dtype=np.int64), np.diff(excl_ptr)) * n_ent + np.asarray(excl_idx, dtype=np.int64)
        live &= ~np.isin(np.arange(n_rows, dtype=np.int64)[:, None] * n_ent + np.where(live, ids, 0), keys)
    c = np.take_along_axis(np.asarray(ci), np.where(live, ids, 0), axis=1)
    pos = np.asarray(pos_int)[:, None]
    return ((c > pos) & live).sum(1), ((c == pos) & live).sum(1), (~live).sum(1)


# ---- ranks on a numpy model ----------------------------------------------------------------------------------------------------------
def cmp_counts(gt, eq, strategy):
    """perform_comparision from the (>, ==) counters"""
    return {"worst": gt + eq, "best": gt, "middle": gt + (eq + 1) // 2}[strategy]


class NumpyModel:
    """DistMult on float32 tables, scored in float64 and rounded once: a model with nothing of the library in it"""

    def __init__(self, n_ent, n_rel, k, seed, copies=6):
        rs = np.random.RandomState(seed)
        self.E = rs.randn(n_ent, k).astype(F32)
        self.R = rs.randn(n_rel, k).astype(F32)
        src, dst = rs.choice(n_ent, size=(2, copies), replace=False)
        self.E[dst] = self.E[src]                                  # entities that tie exactly
        self.copies = list(zip(src.tolist(), dst.tolist()))
        self.n_ent = n_ent

    def side_ci(self, s, p, o, side):
        """comparison integers of every completion of one side of (s, p, o): int64 [n_ent]"""
        fixed = self.E[o] if side == "s" else self.E[s]
        return cmp_int((self.E.astype(np.float64) * (self.R[p].astype(np.float64) * fixed.astype(np.float64))).sum(1)).astype(np.int64)


def known_set(F, s, p, o, side):
    """the filter set of one side of (s, p, o): its own true entity and the known completions"""
    F = np.asarray(F).reshape(-1, 3)
    if side == "o":
        return {int(o)} | set(F[(F[:, 0] == s) & (F[:, 1] == p), 2].tolist())
    return {int(s)} | set(F[(F[:, 2] == o) & (F[:, 1] == p), 0].tolist())


def side_counters(model, T, lists, F, side):
    """per triple the counters of the two statements: walk = (gt, eq) over the entries of the list that are not excluded;
    subset = (gt, eq, fgt, feq) of the entities_subset rule — the whole list, and its members in the filter set"""
    n = len(T)
    walk, subset = np.zeros((2, n), np.int64), np.zeros((4, n), np.int64)
    for i, (s, p, o) in enumerate(np.asarray(T).tolist()):
        ci = model.side_ci(s, p, o, side)
        pos = ci[o if side == "o" else s]
        known = known_set(F, s, p, o, side) if F is not None else set()
        for e in np.asarray(lists[i]).tolist():
            if e < 0 or e >= model.n_ent:
                continue
            g, q = int(ci[e] > pos), int(ci[e] == pos)
            subset[0, i] += g
            subset[1, i] += q
            if e in known:
                subset[2, i] += g
                subset[3, i] += q
            else:
                walk[0, i] += g
                walk[1, i] += q
    return walk, subset


def sampled_ranks(model, T, candidates, F, corrupt_side, strategy):
    """the ranks rank_triples_device(candidates=...) is defined to return: 1 + cmp over the surviving entries of each list"""
    c = {side: side_counters(model, T, candidates[side], F, side)[0] for side in SIDES_OF[corrupt_side]}
    if corrupt_side in ("s", "o"):
        return cmp_counts(c[corrupt_side][0], c[corrupt_side][1], strategy) + 1
    if corrupt_side == "s,o":
        return np.stack([cmp_counts(c["s"][0], c["s"][1], strategy) + 1, cmp_counts(c["o"][0], c["o"][1], strategy) + 1], axis=1)
    return cmp_counts(c["o"][0] + c["s"][0], c["o"][1] + c["s"][1], strategy) + 1


def subset_rank(model, triple, subset, F, side, strategy):
    """rank of ONE triple on one side under the entities_subset rule: cmp(list) + 1 - cmp(filtered members of the list)"""
    _, c = side_counters(model, np.asarray(triple).reshape(1, 3), [subset], F, side)
    return int(cmp_counts(c[0], c[1], strategy)[0] + 1 - cmp_counts(c[2], c[3], strategy)[0])


def toy_graph(n_ent=60, n_rel=5, n=420, seed=17):
    """(train [n, 3], test [24, 3]) int64 ids of a random graph whose test triples share (s, p) and (p, o) pairs with it"""
    rs = np.random.RandomState(seed)
    G = np.unique(np.stack([rs.randint(0, n_ent, n), rs.randint(0, n_rel, n), rs.randint(0, n_ent, n)], 1), axis=0)
    G = G[rs.permutation(len(G))]
    return G[24:], G[:24]
