"""Host statement of the type-constraint contract (emgraph_amd/type_constraints.py, include/emgraph_hip.h: emg_eval_count_grouped
and the pools of emg_sampler), in python sets, numpy and the Philox restatement of tests/_negsample_ref.py.  No device call, and
nothing imported from the code under test.

Pools: group g = 2 p + side, side 0 = the DOMAIN of relation p (its distinct subjects: the candidates when the subject is
corrupted), side 1 = its RANGE (distinct objects); ids ascending; an EMPTY group means "all entities".
Typed counts: per row with group g >= 0, the members of pool g whose comparison integer int32(f32(score) * f32(1e5)) is > / ==
the row's.  Typed draw: the side from attempt 0 as ever; attempt t draws idx_t = mulhi64(o_t[2] << 32 | o_t[1], |pool_g|),
g = 2 p + keep_subject, and takes pool_g[idx_t]; an empty pool (or a relation id out of range) draws as the untyped sampler."""
import numpy as np

from tests._negsample_ref import attempt_index, attempt_words

I32 = np.int32
F32 = np.float32
DOMAIN, RANGE = 0, 1


def pools_from_triples(X, n_rel):
    """(ptr int64 [2 n_rel + 1], idx int32) of the observed pools of the id triples X"""
    groups = [set() for _ in range(2 * n_rel)]
    for s, p, o in np.asarray(X).tolist():
        groups[2 * p + DOMAIN].add(int(s))
        groups[2 * p + RANGE].add(int(o))
    return pools_csr([sorted(g) for g in groups])


def pools_csr(groups):
    """CSR of a list of 2 n_rel id lists ([] = no constraint)"""
    ptr = np.zeros(len(groups) + 1, np.int64)
    ptr[1:] = np.cumsum([len(g) for g in groups])
    idx = np.array([e for g in groups for e in g], dtype=I32)
    return ptr, idx


def pool_of(ptr, idx, g):
    return idx[ptr[g]:ptr[g + 1]]


def cmp_int(score):
    """int32(f32(score) * f32(1e5)) in float32 arithmetic (scores far inside the int32 range)"""
    return (np.asarray(score).astype(F32) * F32(100000.0)).astype(np.int32)


def typed_counts(S, pos_int, row_group, ptr, idx):
    """(gt, eq) int64 [n_rows] from the dense scores S [n_rows, n_ent]: per row the members of its pool that compare > / ==
    pos_int; rows with a negative group, and empty pools, count nothing"""
    ci = cmp_int(S)
    gt, eq = np.zeros(len(ci), np.int64), np.zeros(len(ci), np.int64)
    for r, g in enumerate(np.asarray(row_group).tolist()):
        if g < 0:
            continue
        c = ci[r, pool_of(ptr, idx, g)]
        gt[r], eq[r] = int((c > pos_int[r]).sum()), int((c == pos_int[r]).sum())
    return gt, eq


def row_groups(relations, side, ptr):
    """group per row, -1 where the pool is empty"""
    g = 2 * np.asarray(relations, dtype=np.int64) + side
    return np.where(ptr[g + 1] > ptr[g], g, -1)


def rank_counts(S, pos_int, true_ent, row_group, ptr, idx, known_rows):
    """(gt, eq, fgt, feq) of one side: candidates = the row's pool (all entities for group -1); the filter set of row r is
    ({true_ent[r]} U known_rows[r]) cut down to the candidates (known_rows None: no filter at all)"""
    ci = cmp_int(S)
    n, n_ent = ci.shape
    out = np.zeros((4, n), np.int64)
    for r in range(n):
        g = int(row_group[r])
        cand = np.arange(n_ent) if g < 0 else pool_of(ptr, idx, g)
        c = ci[r, cand]
        out[0, r], out[1, r] = (c > pos_int[r]).sum(), (c == pos_int[r]).sum()
        if known_rows is not None:
            f = sorted((set(known_rows[r]) | {int(true_ent[r])}) & set(np.asarray(cand).tolist()))
            cf = ci[r, f]
            out[2, r], out[3, r] = (cf > pos_int[r]).sum(), (cf == pos_int[r]).sum()
    return out


# ---- typed draws ------------------------------------------------------------------------------------------------------------------
def sample_side_typed(xb, eta, side, seed, counter, n_choices, ptr, idx, n_rel, keep_thr=None, known=None, retries=4, rows=None):
    """tests/_negsample_ref.py::sample_side with pools: dict of ``keep`` / ``repl`` / ``attempt`` / ``left`` / ``typed`` (the row
    drew from a non-empty pool) per row, the ``codes`` and the negatives ``neg``; ``untyped_repl``: the replacement attempt 0 of
    the untyped draw would have given the row"""
    xb = np.asarray(xb, dtype=np.int64)
    B = len(xb)
    j = np.arange(B * int(eta), dtype=np.uint64) if rows is None else np.asarray(rows, dtype=np.uint64)
    n = len(j)
    at = j.astype(np.int64) % B
    T = int(retries) if known is not None else 0
    words = [attempt_words(seed, counter, j, t) for t in range(T + 1)]
    untyped = [attempt_index(w, n_choices) for w in words]
    keep, repl, attempt = np.zeros(n, I32), np.zeros(n, np.int64), np.zeros(n, I32)
    left, typed = np.zeros(n, bool), np.zeros(n, bool)
    for r in range(n):
        s, p, o = (int(v) for v in xb[at[r]])
        in_range = 0 <= p < n_rel
        if side in ("s+o", "s,o"):
            k = int(words[0][0][r]) & 1
            if keep_thr is not None and in_range:
                k = int(int(words[0][3][r]) < int(keep_thr[p]))
        else:
            k = 1 if side == "o" else 0
        pool = pool_of(ptr, idx, 2 * p + k) if in_range else np.zeros(0, I32)
        t = 0
        while True:
            if len(pool):
                e = int(pool[attempt_index((None, words[t][1][r:r + 1], words[t][2][r:r + 1]), len(pool))[0]])
            else:
                e = int(untyped[t][r])
            cand = (s, p, e) if k else (e, p, o)
            inside = known is not None and cand in known
            if not inside or t == T:
                break
            t += 1
        keep[r], repl[r], attempt[r], left[r], typed[r] = k, e, t, inside, len(pool) > 0
    neg = np.stack([np.where(keep == 1, xb[at, 0], repl), xb[at, 1], np.where(keep == 1, repl, xb[at, 2])], 1).astype(I32)
    codes = ((repl & 0x7FFFFFFF) | (keep.astype(np.int64) << 31)).astype(np.uint32).view(I32)
    return dict(keep=keep, repl=repl.astype(I32), attempt=attempt, left=left, typed=typed, codes=codes, neg=neg,
                untyped_repl=np.array(untyped[0], dtype=np.int64), at=at)


def sample_batch_typed(xb, eta, sides, seed, counter0, n_choices, ptr, idx, n_rel, keep_thr=None, known=None, retries=4):
    """every side call of a batch (counter0 + sd), side-major codes, and the four counts"""
    parts = [sample_side_typed(xb, eta, sd, seed, counter0 + i, n_choices, ptr, idx, n_rel, keep_thr, known, retries)
             for i, sd in enumerate(sides)]
    stats = {"rows": sum(len(p["keep"]) for p in parts), "redrawn": sum(int((p["attempt"] > 0).sum()) for p in parts),
             "known_left": sum(int(p["left"].sum()) for p in parts), "typed_rows": sum(int(p["typed"].sum()) for p in parts)}
    return dict(codes=np.concatenate([p["codes"] for p in parts]), neg=[p["neg"] for p in parts], parts=parts, stats=stats)


def outside_pool_share(part, xb, ptr, idx, n_rel):
    """the share of the rows of a side call whose UNTYPED attempt-0 replacement lies outside the row's (non-empty) pool"""
    xb = np.asarray(xb, dtype=np.int64)
    out = 0
    for r in range(len(part["keep"])):
        p = int(xb[part["at"][r], 1])
        if 0 <= p < n_rel:
            pool = pool_of(ptr, idx, 2 * p + int(part["keep"][r]))
            out += int(len(pool) > 0 and int(part["untyped_repl"][r]) not in set(pool.tolist()))
    return out / max(len(part["keep"]), 1)


def fit_reference_typed(X, eta, sides, seed, batches_count, epochs, n_choices, ptr, idx, n_rel, keep_thr=None, known=None, retries=4):
    """tests/_negsample_ref.py::fit_reference with pools: (steps, summed counts)"""
    n = len(X)
    bs = -(-n // batches_count)
    steps, tot = [], {"rows": 0, "redrawn": 0, "known_left": 0, "typed_rows": 0}
    for epoch in range(1, epochs + 1):
        for batch in range(1, batches_count + 1):
            start = (batch - 1) * bs
            B = max(0, min(bs, n - start))
            if B == 0:
                continue
            c0 = ((epoch - 1) * batches_count + (batch - 1)) * len(sides)
            sb = sample_batch_typed(X[start:start + B], eta, sides, seed, c0, n_choices, ptr, idx, n_rel, keep_thr, known, retries)
            for k in tot:
                tot[k] += sb["stats"][k]
            steps.append((epoch, batch, start, B, sb))
    return steps, tot


# ---- the parity table of tests/test_type_constraints.py (API parity) ----------------------------------------------------------------
P_N_ENT, P_N_REL, P_K_INT, P_SEED = 300, 6, 16, 11


def parity_case(seed=P_SEED):
    """dict: tables ``E`` / ``R`` (normal 0.5), a typed training graph ``G`` (relation p: subjects from a window of 120 ids,
    objects from a window of 150), the pool lists ``groups`` observed from G with relation 4's domain and both sides of relation 5
    left unconstrained, 260 test triples ``T`` in shuffled relation order — a fifth of them with an object drawn from ALL entities
    (many outside the range pool) and every tenth with such a subject — and the filter triples ``F`` = G and T together"""
    rs = np.random.RandomState(seed)
    E = (rs.randn(P_N_ENT, P_K_INT) * 0.5).astype(F32)
    R = (rs.randn(P_N_REL, P_K_INT) * 0.5).astype(F32)

    def draw(n, wild_o=0.0, wild_s=0.0):
        p = rs.randint(0, P_N_REL, n)
        s = (20 * p + rs.randint(0, 120, n)) % P_N_ENT
        o = (100 + 20 * p + rs.randint(0, 150, n)) % P_N_ENT
        o = np.where(rs.rand(n) < wild_o, rs.randint(0, P_N_ENT, n), o)
        s = np.where(rs.rand(n) < wild_s, rs.randint(0, P_N_ENT, n), s)
        return np.stack([s, p, o], 1).astype(np.int64)

    G = draw(1500)
    T = draw(260, wild_o=0.2, wild_s=0.1)
    ptr, idx = pools_from_triples(G, P_N_REL)
    groups = [pool_of(ptr, idx, g).tolist() for g in range(2 * P_N_REL)]
    groups[2 * 4 + DOMAIN] = []
    groups[2 * 5 + DOMAIN] = []
    groups[2 * 5 + RANGE] = []
    return dict(E=E, R=R, G=G, T=T, F=np.concatenate([G, T]), groups=groups)


def host_side_counts(model_id, case, side, typed, filtered, scale=1.0):
    """(gt, eq, fgt, feq) [4, n] of one side ('s' / 'o') of the parity table from the C oracle's canonical chain
    (oracle.c_oracle, what tests/_chain_ref.py builds on)"""
    from oracle import c_oracle as co
    E, R, T, F = case["E"], case["R"], case["T"], case["F"]
    ptr, idx = pools_csr(case["groups"])
    k_int = E.shape[1]
    Q, pos_int = co.build_queries(model_id, E, R, k_int, scale, T.astype(I32), 1 if side == "o" else 0)
    S = co.scores_dense(model_id, Q, E, k_int, scale)
    rg = row_groups(T[:, 1], RANGE if side == "o" else DOMAIN, ptr) if typed else np.full(len(T), -1)
    known = None
    if filtered:
        by = {}
        for s, p, o in F.tolist():
            by.setdefault((s, p) if side == "o" else (p, o), set()).add(o if side == "o" else s)
        known = [by.get((s, p) if side == "o" else (p, o), set()) for s, p, o in T.tolist()]
    return rank_counts(S, pos_int, T[:, 2] if side == "o" else T[:, 0], rg, ptr, idx, known)


# ---- the sampler's graphs (3 relations, as tests/_negsample_ref.py) ------------------------------------------------------------------
S_N_ENT, S_N_REL = 1200, 3


def sampler_case(seed=21):
    """dict: pools of 1, 1000, 2, none, 1000 and 2 members (groups 0..5: relation 0's domain is ONE entity, relation 1 has no
    constraint on its objects), 600 triples ``X`` drawn mostly inside them (the filter's known set), the Bernoulli thresholds, and
    300 positives ``xb``"""
    from tests._negsample_ref import keep_thresholds, known_set
    rs = np.random.RandomState(seed)
    groups = [[7], list(range(100, 1100)), [3, 900], [], sorted(rs.choice(S_N_ENT, 1000, replace=False).tolist()), [11, 640]]
    n = 600
    p = rs.randint(0, S_N_REL, n)
    pick = lambda g: np.array(groups[g])[rs.randint(0, len(groups[g]))] if groups[g] else rs.randint(0, S_N_ENT)   # noqa: E731
    s = np.array([pick(2 * q + DOMAIN) if rs.rand() < 0.9 else rs.randint(0, S_N_ENT) for q in p])
    o = np.array([pick(2 * q + RANGE) if rs.rand() < 0.9 else rs.randint(0, S_N_ENT) for q in p])
    X = np.stack([s, p, o], 1).astype(np.int64)
    ptr, idx = pools_csr(groups)
    return dict(X=X, xb=X[:300], groups=groups, ptr=ptr, idx=idx, thr=keep_thresholds(X, S_N_REL), known=known_set(X), n_ent=S_N_ENT)


def fit_graph(seed=31):
    """a typed graph fit() maps itself (labels == ids; every one of the 60 entities occurs): relation p takes its subjects from a
    window of 20 ids and its objects from a window of 25, 898 triples"""
    rs = np.random.RandomState(seed)
    n = 898
    p = rs.randint(0, 3, n)
    s = (15 * p + rs.randint(0, 20, n)) % 60
    o = (30 + 10 * p + rs.randint(0, 25, n)) % 60
    X = np.stack([s, p, o], 1).astype(np.int64)
    assert set(X[:, [0, 2]].ravel().tolist()) == set(range(60))
    return X
