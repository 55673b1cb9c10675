"""Host reference of relation prediction, built only from pieces that were here before it: the relation-side score of
(s, r, o) IS the object-side score — oracle.c_oracle.build_queries(..., EVAL_O) on the expanded triples (s_i, r, o_i), then
oracle.c_oracle.scores_dense against the distinct objects, column o_i.  Counts, exclusions and the total order are numpy
(the order as host_topn of tests/test_topn.py states it).  The C oracle knows TransE-L1 / L2, DistMult, ComplEx and HolE; RotatE
goes through tests/_rotate_ref.chain_f32 on query rows the caller built on the device (rotate_scores); TransE with another
order of the norm has no host oracle and is pinned by the device's own object-side kernels alone (tests/test_relation_ranking.py)."""
import numpy as np

from oracle import c_oracle as co
from oracle import emgraph_oracle as orc
from tests import _rotate_ref as rot

F32 = np.float32
EVAL_O = 1
ORACLE_MODELS = ("TransE_L1", "TransE_L2", "DistMult", "ComplEx", "HolE")


def expand(s, o, cands):
    """int32 [rows * n_cand, 3]: (s_i, r, o_i) for every row i and candidate r, row-major"""
    s, o, cands = (np.asarray(a, np.int64).reshape(-1) for a in (s, o, cands))
    return np.stack([np.repeat(s, len(cands)), np.tile(cands, len(s)), np.repeat(o, len(cands))], 1).astype(np.int32)


def pick_objects(S_all, o, n_cand, objs):
    """[rows, n_cand] from scores [rows * n_cand, len(objs)] of the expanded query rows against the distinct objects"""
    col = np.searchsorted(objs, np.asarray(o, np.int64))
    rows = len(o)
    return S_all.reshape(rows, n_cand, len(objs))[np.arange(rows), :, col]


def scores(model, E, R, k_int, scale, s, o, cands):
    """float32 [rows, n_cand]: the object-side canonical score of (s_i, cands[j], o_i), by the C oracle"""
    assert model in ORACLE_MODELS
    E, R = np.ascontiguousarray(E, F32), np.ascontiguousarray(R, F32)
    T = expand(s, o, cands)
    Q, _ = co.build_queries(orc.MODEL_IDS[model], E, R, k_int, scale, T, EVAL_O)
    objs = np.unique(np.asarray(o, np.int64))
    S_all = co.scores_dense(orc.MODEL_IDS[model], Q, E, k_int, scale, cand=objs.astype(np.int32))
    return pick_objects(S_all, o, len(cands), objs)


def rotate_scores(Q, E, o, n_cand):
    """float32 [rows, n_cand] for RotatE from the query rows Q [rows * n_cand, 2k] the device built for the expanded triples"""
    objs = np.unique(np.asarray(o, np.int64))
    return pick_objects(rot.chain_f32(Q, np.asarray(E, F32)[objs]), o, n_cand, objs)


def cmp_int(x):
    """int32(f32(x) * f32(1e5)) in float32 arithmetic (values far inside the int32 range)"""
    return (np.asarray(x).astype(F32) * F32(100000.0)).astype(np.int32)


def counts(C, pos, cand_ids, excl=None):
    """(gt, eq, fgt, feq) int64 [rows] from comparison integers C [rows, n_cand] of the candidates ``cand_ids``: over every
    candidate, and over the candidates in excl[row]"""
    C, pos = np.asarray(C, np.int64), np.asarray(pos, np.int64)[:, None]
    gt, eq = C > pos, C == pos
    member = np.zeros(C.shape, bool)
    if excl is not None:
        for r, e in enumerate(excl):
            member[r] = np.isin(cand_ids, np.asarray(e, np.int64))
    return gt.sum(1), eq.sum(1), (gt & member).sum(1), (eq & member).sum(1)


def ranks(gt, eq, fgt, feq, strategy):
    """the rank of perform_comparision's three strategies on the four counters, restated"""
    def cmp(g, e):
        return {"worst": g + e, "best": g, "middle": g + (e + 1) // 2}[strategy]
    return cmp(gt, eq) + 1 - cmp(fgt, feq)


def host_topn(S, ids, top_n, excl=None):
    """(ids int32 [rows, N], score bits int32 [rows, N]): higher score first, -0 == +0, NaN last, ties by ascending id, the
    ids in excl[row] left out, short rows padded with (-1, -inf)"""
    rows = S.shape[0]
    out_i = np.full((rows, top_n), -1, np.int32)
    out_s = np.full((rows, top_n), -np.inf, F32)
    ids = np.asarray(ids, np.int64)
    for r in range(rows):
        s = S[r]
        nan = np.isnan(s)
        order = np.lexsort((ids, -(np.where(nan, F32(0), s) + F32(0)), nan))   # last key first: NaN last, score down, id up
        if excl is not None and len(excl[r]):
            order = order[~np.isin(ids[order], excl[r])]
        order = order[:top_n]
        out_i[r, :len(order)] = ids[order]
        out_s[r, :len(order)] = s[order]
    return out_i, out_s.view(np.int32)
