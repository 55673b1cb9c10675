"""Host reference of the sampled corruption draw (include/emgraph_hip.h, emg_sampler_bind): Bernoulli side choice and known-triple
filtering with redraws, restated from the contract on ``oracle.emgraph_oracle.philox4x32_10``, python integers and plain sets.
No device call, nothing imported from the code under test.

Row j of side call sd (counter c = draw_counter0 + sd), attempt t:  o_t = Philox4x32-10((uint32) j, (uint32)(j >> 32) | t << 24,
(uint32) c, (uint32)(c >> 32); seed),  idx_t = mulhi64(o_t[2] << 32 | o_t[1], n_choices).  Side from attempt 0: o_0[0] & 1, or
o_0[3] < keep_thr[p].  Filter: the first attempt whose candidate is not a known triple, the last one if all T + 1 are."""
import numpy as np

from oracle import emgraph_oracle as orc

I32 = np.int32
N_ENT, N_REL = 97, 3
SAT_S, SAT_P = 5, 2            # graph A's planted (s, p): its objects cover every entity


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
    ``known`` None: no filter.  ``rows``: only these draw indices of the call (a sample of a large batch), in this order."""
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
            if not inside or t == T:
                break
            t += 1
        keep[r], repl[r], attempt[r], left[r] = k, e, t, inside
    neg = np.stack([np.where(keep == 1, xb[at, 0], repl), xb[at, 1], np.where(keep == 1, repl, xb[at, 2])], 1).astype(I32)
    codes = ((repl & 0x7FFFFFFF) | (keep.astype(np.int64) << 31)).astype(np.uint32).view(I32)
    return dict(keep=keep, repl=repl.astype(I32), attempt=attempt, left=left, codes=codes, neg=neg)


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
