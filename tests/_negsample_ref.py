"""Host reference of the sampled corruption draw (include/emgraph_hip.h, emg_sampler_bind): Bernoulli side choice and known-triple
filtering with redraws, restated from the contract on ``oracle.emgraph_oracle.philox4x32_10``, python integers and plain sets.
No device call, nothing imported from the code under test.

Row j of side call sd (counter c = draw_counter0 + sd), attempt t:  o_t = Philox4x32-10((uint32) j, (uint32)(j >> 32) | t << 24,
(uint32) c, (uint32)(c >> 32); seed),  idx_t = mulhi64(o_t[2] << 32 | o_t[1], n_choices).  Side from attempt 0: o_0[0] & 1, or
o_0[3] < keep_thr[p].  Filter: the first attempt whose candidate is not a known triple, the last one if all T + 1 are.

Graph A (97 entities, 898 triples: the whole known set is the filter's coarse index, every key below 2^17) and Graph B (``graph_b``:
1024 .. 60001 known triples over the lowest and the highest ids of a table of 262149 rows: the bind's shift is 0, 1, 2, 3 and 6, the
keys lie on both sides of 2^32), with the host restatement of the bind's rule (``coarse_index``), the key of a triple (``triple_keys``)
and the candidates a side call examined (``sample_side``'s ``examined``)."""
import functools

import numpy as np

from oracle import emgraph_oracle as orc

I32 = np.int32
N_ENT, N_REL = 97, 3
SAT_S, SAT_P = 5, 2            # graph A's planted (s, p): its objects cover every entity
N_ENT_B = 262144 + 5           # graph B's table: just tall enough for the bucket form of emg_prepare_batch
COARSE_MAX = 1024              # csrc/emg_sampler.hpp, kCoarseMax
# graph B's sizes (n_known, n_ids): 1024 the last with the whole set in the coarse index; 1025: the final run holds one key;
# 5403 and 60001: no multiples of 2^shift
SIZES_B = ((1024, 60), (1025, 60), (2049, 60), (5403, 60), (60001, 200))
SHIFTS_B = (0, 1, 2, 3, 6)


def keep_thresholds(X, n_rel):
    """keep_thr[p] = min(2^32 - 1, floor(|S_p| 2^32 / (|S_p| + |O_p|))) in exact integers; 2^31 for a relation without triples"""
    out = []
    for p in range(n_rel):
        rows = [(int(s), int(o)) for s, pp, o in np.asarray(X).tolist() if pp == p]
        a, b = len({s for s, _ in rows}), len({o for _, o in rows})
        out.append(min((1 << 32) - 1, (a << 32) // (a + b)) if a + b else 1 << 31)
    return np.array(out, dtype=np.uint32)


def known_set(X):
    return {(int(s), int(p), int(o)) for s, p, o in np.asarray(X).tolist()}


def attempt_words(seed, counter, j, t):
    """the four Philox words of attempt ``t`` for the draw indices ``j`` (uint64 array)"""
    j = np.asarray(j, dtype=np.uint64)
    seed, counter = int(seed) & 0xFFFFFFFFFFFFFFFF, int(counter) & 0xFFFFFFFFFFFFFFFF
    c1 = (j >> np.uint64(32)).astype(np.uint32) | np.uint32((int(t) << 24) & 0xFFFFFFFF)
    return orc.philox4x32_10((j & np.uint64(0xFFFFFFFF)).astype(np.uint32), c1, np.uint32(counter & 0xFFFFFFFF),
                             np.uint32(counter >> 32), np.uint32(seed & 0xFFFFFFFF), np.uint32(seed >> 32))


def attempt_index(words, n_choices):
    n = int(n_choices)
    return [(((int(o2) << 32) | int(o1)) * n) >> 64 for o1, o2 in zip(words[1].tolist(), words[2].tolist())]


def sample_side(xb, eta, side, seed, counter, n_choices, pool=None, keep_thr=None, known=None, retries=4, rows=None):
    """One side call over the positives ``xb`` [B, 3] (row j corrupts positive j mod B): dict of ``keep`` / ``repl`` /
    ``attempt`` (final attempt) / ``left`` (final candidate known) per row, the ``codes`` (repl | keep << 31, int32) and the
    negatives ``neg`` [B * eta, 3].  ``pool``: the replacement-id mapping (None: the identity); ``keep_thr`` None: uniform side;
    ``known`` None: no filter.  ``rows``: only these draw indices of the call (a sample of a large batch), in this order.
    With a filter also ``examined`` [m, 4]: every candidate (s, p, o, known) the search looked up, over all attempts."""
    xb = np.asarray(xb, dtype=np.int64)
    B = len(xb)
    j = np.arange(B * int(eta), dtype=np.uint64) if rows is None else np.asarray(rows, dtype=np.uint64)
    n = len(j)
    at = j.astype(np.int64) % B                      # the positive each row corrupts
    words = [attempt_words(seed, counter, j, 0)]
    idx = [attempt_index(words[0], n_choices)]
    T = int(retries) if known is not None else 0
    for t in range(1, T + 1):
        words.append(attempt_words(seed, counter, j, t))
        idx.append(attempt_index(words[t], n_choices))
    mapped = (lambda i: int(pool[i])) if pool is not None else (lambda i: int(i))
    keep, repl, attempt, left = np.zeros(n, I32), np.zeros(n, np.int64), np.zeros(n, I32), np.zeros(n, bool)
    examined = []
    for r in range(n):
        s, p, o = (int(v) for v in xb[at[r]])
        if side in ("s+o", "s,o"):
            k = int(words[0][0][r]) & 1 if keep_thr is None else int(int(words[0][3][r]) < int(keep_thr[p]))
        else:
            k = 1 if side == "o" else 0
        t = 0
        while True:
            e = mapped(idx[t][r])
            cand = (s, p, e) if k else (e, p, o)
            inside = known is not None and cand in known
            if known is not None:
                examined.append(cand + (int(inside),))
            if not inside or t == T:
                break
            t += 1
        keep[r], repl[r], attempt[r], left[r] = k, e, t, inside
    neg = np.stack([np.where(keep == 1, xb[at, 0], repl), xb[at, 1], np.where(keep == 1, repl, xb[at, 2])], 1).astype(I32)
    codes = ((repl & 0x7FFFFFFF) | (keep.astype(np.int64) << 31)).astype(np.uint32).view(I32)
    return dict(keep=keep, repl=repl.astype(I32), attempt=attempt, left=left, codes=codes, neg=neg,
                examined=np.array(examined, dtype=np.int64).reshape(-1, 4))


def sample_batch(xb, eta, sides, seed, counter0, n_choices, pool=None, keep_thr=None, known=None, retries=4):
    """every side call of a batch (counter0 + sd), as emg_prepare_batch lays them out: side-major codes / negatives and the three
    counts {rows, redrawn, known_left}"""
    parts = [sample_side(xb, eta, sd, seed, counter0 + i, n_choices, pool, keep_thr, known, retries) for i, sd in enumerate(sides)]
    stats = {"rows": sum(len(p["keep"]) for p in parts), "redrawn": sum(int((p["attempt"] > 0).sum()) for p in parts),
             "known_left": sum(int(p["left"].sum()) for p in parts)}
    return dict(codes=np.concatenate([p["codes"] for p in parts]), neg=[p["neg"] for p in parts], parts=parts, stats=stats)


def graph_a(seed=0):
    """Graph A: 97 entities, 3 relations, 898 distinct triples in a seeded random order — relation 0 pure 1-to-N (4 subjects share
    the 97 objects), relation 1 pure N-to-1 (its mirror), relation 2 random, with the planted (SAT_S, SAT_P) whose objects are ALL
    entities: an object corruption of one of its triples can never leave the known set."""
    rs = np.random.RandomState(1234 + seed)
    ents = np.arange(N_ENT)
    one_to_n = np.stack([ents % 4, np.zeros(N_ENT, int), ents], 1)
    n_to_one = np.stack([ents, np.ones(N_ENT, int), 10 + ents % 4], 1)
    planted = np.stack([np.full(N_ENT, SAT_S), np.full(N_ENT, SAT_P), ents], 1)
    have = known_set(planted)
    rnd = []
    while len(rnd) < 898 - 3 * N_ENT:
        t = (int(rs.randint(0, N_ENT)), SAT_P, int(rs.randint(0, N_ENT)))
        if t not in have:
            have.add(t)
            rnd.append(t)
    X = np.concatenate([one_to_n, n_to_one, planted, np.array(rnd)], 0).astype(np.int64)
    return X[rs.permutation(len(X))]


# ---- Graph B: the filter's second level and 64-bit keys ----------------------------------------------------------------------------
def coarse_index(n_known):
    """(shift, n_coarse) as emg_sampler_bind picks them: the smallest shift with ceil(n_known / 2^shift) <= COARSE_MAX"""
    shift = 0
    while -(-int(n_known) // (1 << shift)) > COARSE_MAX:
        shift += 1
    return shift, -(-int(n_known) // (1 << shift))


def triple_keys(T, n_ent, n_rel):
    """the keys (s * n_rel + p) * n_ent + o of the triples T [n, >= 3] in python integers"""
    return [(int(s) * int(n_rel) + int(p)) * int(n_ent) + int(o) for s, p, o in np.asarray(T)[:, :3].tolist()]


def ids_b(n_ids):
    """the n_ids / 2 lowest and the n_ids / 2 highest entities of graph B's table, ascending"""
    h = int(n_ids) // 2
    return np.concatenate([np.arange(h), np.arange(N_ENT_B - h, N_ENT_B)]).astype(np.int64)


def graph_b(n_known, n_ids=60, seed=4321):
    """Graph B: the first ``n_known`` of the seeded permutation of ALL combinations (s, p, o) over ``ids_b(n_ids)`` and 3 relations —
    a dense graph (a draw from the ids hits a known triple with probability n_known / (3 n_ids^2)) whose low subjects give keys
    below 2^32 and whose high subjects keys near 2 * 10^11"""
    ids = ids_b(n_ids)
    n = len(ids)
    assert 0 < n_known <= 3 * n * n
    c = np.random.RandomState(seed).permutation(3 * n * n)[:n_known]
    return np.stack([ids[c // (3 * n)], (c // n) % 3, ids[c % n]], 1).astype(np.int64)


@functools.lru_cache(maxsize=None)
def case_b(n_known, n_ids=60, seed=4321):
    """a bound set of graph B with what its tests share (built once; nobody writes to it): the triples ``X``, the set ``known``,
    the Bernoulli thresholds ``thr``, the corruption ``pool`` (the ids in REVERSE order: entities_list, n_choices = n_ids) and the
    positives ``xb`` (the first 300 triples)"""
    X = graph_b(n_known, n_ids, seed)
    return dict(X=X, known=known_set(X), thr=keep_thresholds(X, N_REL), ids=ids_b(n_ids), pool=ids_b(n_ids)[::-1].astype(I32).copy(),
                xb=X[:300], n_ent=N_ENT_B, n_known=n_known)


def corner_positives(ids):
    """300 positives around the pool's extreme combinations (lo, 0, lo) and (hi, 2, hi): (lo, 0, x), (x, 0, lo), (hi, 2, x), (x, 2, hi)
    in turn, x running over the ids — a draw of lo / hi for the replaced side gives the smallest / largest key a candidate of this
    pool can have"""
    lo, hi = int(ids[0]), int(ids[-1])
    rows = []
    for i in range(300):
        x = int(ids[(7 * i) % len(ids)])
        rows.append(((lo, 0, x), (x, 0, lo), (hi, 2, x), (x, 2, hi))[i % 4])
    return np.array(rows, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def corner_cases_b():
    """the corner bindings over the 60 ids of graph B, name -> case (as ``case_b``; the positives are ``corner_positives``, the
    pool the 4 lowest and the 4 highest ids in reverse order, so that the extreme combinations are drawn often):
    'one_low' / 'one_high': ONE known key, the smallest / the largest a candidate can have (a search hits entry 0, passes it or —
    'one_high' — falls off the low end); 'absent' / 'present': 2049 keys without the two extreme combinations, and the same set
    with both added (2051 keys)"""
    ids = ids_b(60)
    lo, hi = (int(ids[0]), 0, int(ids[0])), (int(ids[-1]), 2, int(ids[-1]))
    absent = np.array([t for t in graph_b(2060, 60, 99).tolist() if tuple(t) not in (lo, hi)][:2049], dtype=np.int64)
    present = np.concatenate([absent, np.array([lo, hi], dtype=np.int64)])
    out = {}
    for name, X in (("one_low", np.array([lo], dtype=np.int64)), ("one_high", np.array([hi], dtype=np.int64)), ("absent", absent),
                    ("present", present)):
        out[name] = dict(X=X, known=known_set(X), thr=keep_thresholds(X, N_REL), ids=ids, pool=ids_b(8)[::-1].astype(I32).copy(),
                         xb=corner_positives(ids), n_ent=N_ENT_B, n_known=len(X), lo=lo, hi=hi)
    return out


def graph_fit_b(seed=4321):
    """the dense graph fit() maps itself (labels == ids): 60 entities, 3 relations, 5403 of the 10800 combinations (shift = 3)"""
    c = np.random.RandomState(seed).permutation(3 * 60 * 60)[:5403]
    return np.stack([c // 180, (c // 60) % 3, c % 60], 1).astype(np.int64)


def examined_counts(parts, n_ent, n_rel):
    """{(key >= 2^32, known): number of examined candidates} over the side calls ``parts``"""
    out = {(hi, kn): 0 for hi in (False, True) for kn in (False, True)}
    for p in parts:
        for key, kn in zip(triple_keys(p["examined"], n_ent, n_rel), p["examined"][:, 3].tolist()):
            out[(key >= 1 << 32, bool(kn))] += 1
    return out


def check_not_vacuous(case, want, retries):
    """the conditions under which a comparison with ``want`` (a ``sample_batch`` over ``case``) tests the filter's second level
    and its 64-bit keys, from the reference alone: the bind's shift is >= 1 past 1024 keys; the known keys and the examined
    candidates — known ones and unknown ones — lie on both sides of 2^32; at least 5 % of the rows are redrawn and some are not;
    from 5403 keys on rows are left known and every final attempt 0..T occurs"""
    n_known = case["n_known"]
    assert coarse_index(n_known)[0] >= 1 or n_known <= COARSE_MAX
    keys = triple_keys(case["X"], case["n_ent"], N_REL)
    assert min(keys) < 1 << 32 <= max(keys)
    ex = examined_counts(want["parts"], case["n_ent"], N_REL)
    assert all(v > 0 for v in ex.values()), ex
    st = want["stats"]
    attempt = np.concatenate([p["attempt"] for p in want["parts"]])
    assert 20 * st["redrawn"] >= st["rows"] and (attempt == 0).any(), st
    if n_known >= 5403:
        assert st["known_left"] > 0 and set(attempt.tolist()) == set(range(retries + 1)), (st, sorted(set(attempt.tolist())))


def fit_reference(X, eta, sides, seed, batches_count, epochs, n_choices, pool=None, keep_thr=None, known=None, retries=4):
    """the negatives of every step of a fit() (batch size ceil(n / batches_count), counter0 = ((epoch - 1) * batches_count +
    batch - 1) * len(sides)): list of (epoch, batch, start, B, sample_batch(...)) and the summed counts"""
    n = len(X)
    bs = -(-n // batches_count)
    steps, tot = [], {"rows": 0, "redrawn": 0, "known_left": 0}
    for epoch in range(1, epochs + 1):
        for batch in range(1, batches_count + 1):
            start = (batch - 1) * bs
            B = max(0, min(bs, n - start))
            if B == 0:
                continue
            c0 = ((epoch - 1) * batches_count + (batch - 1)) * len(sides)
            xb = X[start:start + B]
            pl = pool(xb) if callable(pool) else pool        # ('batch': the pool is the batch's own entities)
            sb = sample_batch(xb, eta, sides, seed, c0, len(pl) if callable(pool) else n_choices, pl, keep_thr, known, retries)
            for k in tot:
                tot[k] += sb["stats"][k]
            steps.append((epoch, batch, start, B, sb))
    return steps, tot
