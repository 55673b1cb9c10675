"""Hand-made pair lists for the exact re-scoring kernels (csrc/emg_rank.hip: rescore_pairs_kernel, rescore_segment_kernel, the tile
form) and their expected counters.  Host only: numpy and the C oracle's explicit-fmaf chain, no torch, no device.

A case is tables (E, Q), the positives' comparison integers and a pair buffer in the prefilter's layout: n_seg segments of cap
entries, entry = (row << 32) | global entity id, pair_count[s] the number of entries segment s holds (a count above cap means the
segment overflowed: its first cap entries are read), pair_count[n_seg] the overflow flag the re-scoring never reads.

The LAST query row is the sentinel: no counted pair names it, every padding entry behind a segment's count names it with an
in-range entity, and its positive is INT32_MIN, so a kernel that reads past a count moves the sentinel's `>` counter instead of
leaving the buffers.  Every row and entity id in every buffer, padding included, is in range."""
import functools
from types import SimpleNamespace

import numpy as np

from oracle import c_oracle as co

F32 = np.float32
TRANSE_L1, TRANSE_L2, DISTMULT, COMPLEX, HOLE = range(5)   # EMG_* model ids (tests/test_rescore_host.py pins them to _lib's)
MODELS = {"TransE_L1": TRANSE_L1, "TransE_L2": TRANSE_L2, "DistMult": DISTMULT, "ComplEx": COMPLEX, "HolE": HOLE}
LINKS = ("linear", "tanh", "sigmoid", "softplus")           # EMG_LINK_* 0..3

N_ROWS, N_ENT, N_SEG, CAP = 130, 200, 27, 1600              # four 32-row blocks and a part + the sentinel; a last 32-row tile of 8
ENT_TILE = 128                                              # the prefilter lists a segment's pairs by tiles of 128 entities
RQ_ROWS = 32                                                # rows of the LDS image (rescore_segment_kernel)
WIDTHS = (4, 20, 32, 36, 64, 68, 200, 576, 864)             # the vector forms (see tests/test_rescore.py)
TILE_WIDTHS = (4, 36, 200, 576)
LINK_WIDTHS = (36, 200, 576)
LINK_MODELS = ("DistMult", "ComplEx", "TransE_L1")
SCALAR_SHAPES = ((37, 37, 0), (36, 39, 0), (36, 48, 1))     # (k_int, ld, floats past a 16-byte boundary)
BIG_N_LOCAL = 262144 + 40                                   # tile_scan_kernel's second loop trip: more than 8192 tiles of 32 rows
BIG_TILES = (0, 8191, 8192, 8193)                           # 8193: the last tile, 8 rows

# (count word, rows of the segment, entity order); one entry per segment.  Long segments (>= 512 pairs): each span kind and each
# order at least twice.  CAP + 5: a segment that overflowed.
SEGMENTS = (
    (0, "span32", "ascending"), (1, "scattered", "ascending"), (63, "span32", "random"), (64, "span33", "rotated"),
    (65, "scattered", "random"), (255, "span_exact", "rotated"), (256, "span32", "rotated"), (257, "span33", "ascending"),
    (511, "one_row", "random"), (512, "span32", "rotated"), (513, "span33", "ascending"), (CAP, "span_exact", "random"),
    (CAP + 5, "scattered", "rotated"), (600, "one_row", "ascending"), (700, "span32", "random"), (777, "span_exact", "rotated"),
    (900, "span33", "random"), (1024, "scattered", "ascending"), (1300, "one_row", "rotated"), (0, "scattered", "random"),
    (17, "span_exact", "ascending"), (128, "one_row", "rotated"), (300, "span_exact", "ascending"), (400, "scattered", "random"),
    (200, "span33", "random"), (2, "span32", "ascending"), (1111, "span_exact", "ascending"),
)
assert len(SEGMENTS) == N_SEG and N_SEG % 4 and N_SEG % 8
SPANS = ("span32", "span_exact", "span33", "scattered", "one_row")
ORDERS = ("ascending", "rotated", "random")


def hole_scale(k_int):
    """HolE's 2 / k with k = k_int / 2 complex coordinates"""
    return float(F32(4.0) / F32(k_int))


def table_scale(model, k_int, linked=False):
    """standard deviation of the table entries.  Unlinked: scores of order one to ten.  Linked: contraction scores with a standard
    deviation of ~5 (tanh and the sigmoid saturate for a share of the pairs of every row), TransE-L1 scores around -2"""
    if not linked:
        return 0.3
    if model == TRANSE_L1:
        return 2.0 / (1.13 * np.sqrt(2.0) * k_int)   # E|q - e| = 1.13 sigma sqrt(2)
    return float(np.sqrt(5.0 / np.sqrt(k_int)))


# ---- the comparison integer --------------------------------------------------------------------------------------------------------
def cmp_int(S):
    """int32(score * 1e5), the product in float32, truncated; the scores must leave the cast defined"""
    S = np.asarray(S, F32)
    assert not np.isnan(S).any() and (np.abs(S.astype(np.float64)) * 1e5 < 2 ** 31 - 1000).all()
    return (S * F32(100000.0)).astype(np.int32)


def link_value(link, S):
    """phi(score) in float32 (numpy's libm, not the device's: used to CHOOSE positives for the linked cases, never to expect)"""
    S = np.asarray(S, F32)
    if link == "tanh":
        return np.tanh(S).astype(F32)
    if link == "sigmoid":
        return (F32(1) / (F32(1) + np.exp(-S))).astype(F32)
    if link == "softplus":                      # the reference's custom_softplus, log(1 + 9999 e^x)
        return np.log(F32(1) + F32(9999) * np.exp(S)).astype(F32)
    return S


# ---- segment builders ----------------------------------------------------------------------------------------------------------------
def _rows_of(kind, n, rs, n_counted):
    """(n query rows of a segment, all below n_counted — the sentinel is n_counted —, the positions that pin the span's two ends)"""
    pin = rs.choice(n, 2, replace=False) if n >= 2 else np.zeros(0, np.int64)
    if n == 0:
        return np.zeros(0, np.int64), pin
    if kind == "one_row":
        return np.full(n, rs.randint(0, n_counted), np.int64), pin[:0]
    if kind == "span32":                      # inside one aligned block of 32 rows
        b = 32 * rs.randint(0, n_counted // 32)
        r, ends = b + rs.randint(0, 32, n), (b + 3, b + 30)
    elif kind == "span_exact":                # min and max exactly 31 apart, the block unaligned
        b = 1 + rs.randint(0, n_counted - 33)
        b += (b % 32 == 0)
        r, ends = b + rs.randint(0, 32, n), (b, b + 31)
    elif kind == "span33":                    # min and max 32 apart: the first span the LDS image does not hold
        b = rs.randint(0, n_counted - 32)
        r, ends = b + rs.randint(0, 33, n), (b, b + 32)
    else:                                     # scattered over every counted row
        r, ends = rs.randint(0, n_counted, n), (0, n_counted - 1)
    if n >= 2:
        r[pin] = ends
    return r.astype(np.int64), pin


def _order(order, e, rs, tile=ENT_TILE):
    """a permutation of the segment's pairs by the tile of their entity"""
    n = len(e)
    perm = rs.permutation(n)
    if order == "random" or n == 0:
        return perm
    t = e[perm] // tile
    asc = perm[np.argsort(t, kind="stable")]            # tiles ascending, any order inside a tile
    if order == "ascending":
        return asc
    ts = np.unique(t)
    first = ts[len(ts) // 2] if len(ts) > 1 else ts[0]  # rotated: from tile `first` to the end, then from tile 0
    ta = e[asc] // tile
    return np.concatenate([asc[ta >= first], asc[ta < first]])


def _segment(n, kind, order, rs, n_counted, ents, true_of, dup):
    """(rows, local entities) of one segment's n counted pairs; `ents`: the entities a pair may name; every seventh pair names its
    row's true entity (or the true entity's copy: a tie); dup: a tenth of the pairs repeat another pair of the segment"""
    r, pin = _rows_of(kind, n, rs, n_counted)
    e = ents[rs.randint(0, len(ents), n)].astype(np.int64)
    if true_of is not None and n:
        hit = rs.rand(n) < 1.0 / 7.0
        e[hit] = true_of[rs.randint(0, 2, hit.sum()), r[hit]]
    if dup and n >= 10:
        free = np.setdiff1d(np.arange(n), pin)              # the span's two end rows stay
        dst = rs.choice(free, n // 10, replace=False)
        src = rs.choice(np.setdiff1d(np.arange(n), dst), n // 10)
        r[dst], e[dst] = r[src], e[src]
    p = _order(order, e, rs)
    return r[p], e[p]


def _tables(model, k_int, seed, scale, n_rows, n_ent, n_copies=40):
    rs = np.random.RandomState(seed)
    E = (rs.randn(n_ent, k_int) * scale).astype(F32)
    Q = (rs.randn(n_rows, k_int) * scale).astype(F32)
    pick = rs.choice(n_ent, 2 * n_copies, replace=False)
    src, dst = pick[:n_copies], pick[n_copies:]
    E[dst] = E[src]                                        # exact copies: candidates that tie
    # the true entity of row r, and its copy (itself where it has none); every third row's true entity has one
    true_of = np.empty((2, n_rows), np.int64)
    plain = np.setdiff1d(np.arange(n_ent), pick)
    for r in range(n_rows):
        if r % 3 == 0:
            j = rs.randint(0, n_copies)
            true_of[:, r] = src[j], dst[j]
        else:
            true_of[:, r] = plain[rs.randint(0, len(plain))]
    return E, Q, true_of


def _finish(model, k_int, scale, link, E, Q, true_of, seg_rows, seg_ents, counts, cap, n_rows, ent_offset, meta):
    n_seg = len(counts)
    sentinel = n_rows - 1
    rs = np.random.RandomState(k_int + 17)
    pairs = (np.int64(sentinel) << 32) | (rs.randint(0, E.shape[0], (n_seg, cap)).astype(np.int64) + ent_offset)
    for s in range(n_seg):
        m = len(seg_rows[s])
        assert m == min(counts[s], cap) and (seg_rows[s] < sentinel).all() and (seg_rows[s] >= 0).all()
        assert (seg_ents[s] >= 0).all() and (seg_ents[s] < E.shape[0]).all()
        pairs[s, :m] = (seg_rows[s] << 32) | (seg_ents[s] + ent_offset)
    pos, true_score = np.empty(n_rows, np.int32), np.empty(n_rows, F32)
    for r in range(n_rows):
        true_score[r] = co.scores_dense(model, Q[r:r + 1], E, k_int, scale, cand=true_of[:1, r].astype(np.int32))[0, 0]
        pos[r] = cmp_int(link_value(link, true_score[r:r + 1]))[0]
    pos[sentinel] = np.iinfo(np.int32).min
    return SimpleNamespace(model=model, k_int=k_int, scale=scale, link=link, E=E, Q=Q, pos_int=pos, true_score=true_score, pairs=pairs,
                           pair_count=np.array(list(counts) + [0], np.int32), ent_offset=ent_offset, cap=cap, n_seg=n_seg,
                           n_rows=n_rows, sentinel=sentinel, seg_kind=[m[0] for m in meta], seg_order=[m[1] for m in meta])


@functools.lru_cache(maxsize=None)
def segment_case(model_name, k_int, link="linear"):
    """the case of (model, width): SEGMENTS in an order drawn from the seed, duplicates in every second segment"""
    model = MODELS[model_name]
    seed = 1000 * model + k_int + 50000 * LINKS.index(link)
    scale = hole_scale(k_int) if model == HOLE else 1.0
    E, Q, true_of = _tables(model, k_int, seed, table_scale(model, k_int, link != "linear"), N_ROWS, N_ENT)
    rs = np.random.RandomState(seed + 1)
    order = rs.permutation(N_SEG)
    rows, ents, counts, meta = [], [], [], []
    for s in order:
        cnt, kind, eo = SEGMENTS[s]
        r, e = _segment(min(cnt, CAP), kind, eo, rs, N_ROWS - 1, np.arange(N_ENT), true_of, dup=bool(s % 2 == 0))
        rows.append(r); ents.append(e); counts.append(cnt); meta.append((kind, eo))
    return _finish(model, k_int, scale, link, E, Q, true_of, rows, ents, counts, CAP, N_ROWS, 0, meta)


@functools.lru_cache(maxsize=None)
def big_tile_case(model_name="ComplEx", k_int=4):
    """BIG_N_LOCAL entities (a 4 MB table at k_int 4), a few hundred pairs in each of BIG_TILES: tile_scan_kernel's second loop trip"""
    model = MODELS[model_name]
    n_seg, cap = 6, 256
    E, Q, true_of = _tables(model, k_int, 4242, 0.5, N_ROWS, BIG_N_LOCAL)
    rs = np.random.RandomState(4243)
    tiles = [np.arange(32 * t, min(32 * t + 32, BIG_N_LOCAL)) for t in BIG_TILES]
    pool = np.concatenate(tiles)
    draw = np.concatenate([np.tile(t, 32 // len(t)) for t in tiles])   # every tile named equally often
    for r in range(N_ROWS):                                 # the true entities move into the tiles the pairs name
        j = rs.randint(0, len(pool) - 1)
        true_of[:, r] = pool[j], pool[j]
        if r % 3 == 0:
            E[pool[j + 1]] = E[pool[j]]
            true_of[1, r] = pool[j + 1]
    rows, ents, counts, meta = [], [], [], []
    for s, cnt in enumerate((200, 256, 0, 131, 77, 255)):
        r, e = _segment(cnt, "scattered", "ascending", rs, N_ROWS - 1, draw, true_of, dup=bool(s % 2))
        p = np.argsort(e // 32, kind="stable")
        rows.append(r[p]); ents.append(e[p]); counts.append(cnt); meta.append(("scattered", "ascending"))
    return _finish(model, k_int, 1.0, "linear", E, Q, true_of, rows, ents, counts, cap, N_ROWS, 0, meta)


def with_offset(case, ent_offset):
    """the same case as a slab that starts at global entity `ent_offset`: global ids in the pairs"""
    c = SimpleNamespace(**vars(case))
    c.pairs = case.pairs + np.int64(ent_offset - case.ent_offset)
    c.ent_offset = ent_offset
    return c


# ---- expected counters -------------------------------------------------------------------------------------------------------------
def counted(case):
    """per segment the (rows, local entities) of its first min(count, cap) entries"""
    out = []
    for s in range(case.n_seg):
        w = case.pairs[s, :min(int(case.pair_count[s]), case.cap)]
        out.append((w >> 32, (w & 0xffffffff) - case.ent_offset))
    return out


def expected(case):
    """(gt, eq) int64 [n_rows]: what the counted pairs add to the counters under the LINEAR link; scores from the oracle's
    k-ordered chain, row by row over the row's own entities (never a dense n_rows x n_ent matrix)"""
    segs = counted(case)
    rows = np.concatenate([s[0] for s in segs])
    ents = np.concatenate([s[1] for s in segs])
    gt, eq = np.zeros(case.n_rows, np.int64), np.zeros(case.n_rows, np.int64)
    for r in np.unique(rows):
        cand = ents[rows == r].astype(np.int32)
        ci = cmp_int(co.scores_dense(case.model, case.Q[r:r + 1], case.E, case.k_int, case.scale, cand=cand))[0]
        gt[r], eq[r] = (ci > case.pos_int[r]).sum(), (ci == case.pos_int[r]).sum()
    return gt, eq


def as_csr(case):
    """the counted pairs as eval_filter_count's per-row CSR: (ptr int64 [n_rows + 1], idx int32 global ids, repeats kept)"""
    segs = counted(case)
    rows = np.concatenate([s[0] for s in segs])
    ents = np.concatenate([s[1] for s in segs]) + case.ent_offset
    o = np.argsort(rows, kind="stable")
    ptr = np.zeros(case.n_rows + 1, np.int64)
    ptr[1:] = np.cumsum(np.bincount(rows, minlength=case.n_rows))
    return ptr, ents[o].astype(np.int32)


# ---- what a case exercises ---------------------------------------------------------------------------------------------------------
def span_kind(rows):
    """the builder a segment's rows satisfy, read from the rows"""
    if len(rows) == 0:
        return None
    lo, hi = int(rows.min()), int(rows.max())
    if lo == hi:
        return "one_row"
    if lo // 32 == hi // 32:
        return "span32"
    if hi - lo == 31:
        return "span_exact"
    if hi - lo == 32:
        return "span33"
    return "scattered"


def entity_order(ents, tile=ENT_TILE):
    """ascending | rotated | random, read from the tiles of a segment's entities; None where fewer than two tiles appear"""
    t = ents // tile
    down = np.flatnonzero(t[1:] < t[:-1])
    if len(np.unique(t)) < 2:
        return None
    if len(down) == 0:
        return "ascending"
    if len(down) == 1 and t[-1] < t[0]:
        return "rotated"
    return "random"


def coverage(case, min_long=512):
    """what a case exercises, read from its buffers (min_long: the LDS form's threshold at the case's width)"""
    segs = counted(case)
    n = np.array([len(s[0]) for s in segs])
    gt, eq = expected(case)
    long_ = [s for s in segs if len(s[0]) >= min_long]
    spans = [span_kind(s[0]) for s in long_]
    orders = [entity_order(s[1]) for s in long_]
    dups = 0
    for r, e in segs:
        w = (r << 32) | e
        dups += len(w) - len(np.unique(w))
    words = (case.pairs >> 32)
    return dict(
        sizes=sorted(int(x) for x in case.pair_count[:case.n_seg]),
        below_256=int(((n >= 1) & (n < 256)).sum()), from_256_below_512=int(((n >= 256) & (n < 512)).sum()),
        from_512=int((n >= 512).sum()), long=len(long_),
        wraps=sum(1 for s in long_ if (np.diff(s[1] // ENT_TILE) < 0).any()),
        staged=sum(1 for s in long_ if s[0].max() - s[0].min() + 1 <= RQ_ROWS),
        unstaged=sum(1 for s in long_ if s[0].max() - s[0].min() + 1 > RQ_ROWS),
        spans={k: spans.count(k) for k in SPANS}, orders={k: orders.count(k) for k in ORDERS},
        rows_gt=int((gt > 0).sum()), rows_eq=int((eq > 0).sum()), duplicates=int(dups),
        truncated=bool((case.pair_count[:case.n_seg] > case.cap).any()),
        sentinel_counted=int(sum((s[0] == case.sentinel).sum() for s in segs)),
        sentinel_padding=bool(all((words[s, len(segs[s][0]):] == case.sentinel).all() for s in range(case.n_seg))),
        in_range=bool((words >= 0).all() and (words < case.n_rows).all()
                      and ((case.pairs & 0xffffffff) >= case.ent_offset).all()
                      and ((case.pairs & 0xffffffff) < case.ent_offset + case.E.shape[0]).all()),
    )


# ---- the LDS image's limits, read from the source ----------------------------------------------------------------------------------
def lds_limits(source):
    """(RQ_ROWS, RQ_LD, RQ_LDS_MAX, RQ_MIN_PAIRS) parsed from csrc/emg_rank.hip"""
    import re

    def const(name):
        m = re.search(r"constexpr int [^;]*\b%s = ([^,;]+)[,;]" % name, source)
        assert m, name
        return m.group(1).strip()
    kc = int(const("RQ_KC"))
    ld = const("RQ_LD")
    assert ld == "RQ_KC + 4"
    mx = const("RQ_LDS_MAX")
    assert re.fullmatch(r"\d+ \* 1024", mx)
    assert "return ((size_t)RQ_ROWS * (k_int + 4) + (size_t)waves * 64 * RQ_LD) * sizeof(float);" in source
    return int(const("RQ_ROWS")), kc + 4, int(mx.split()[0]) * 1024, int(const("RQ_MIN_PAIRS"))


def image_waves(k_int, limits):
    """rescore_image_waves: 8 | 4 | 0 waves at this width"""
    rows, ld, lds_max, _ = limits
    for w in (8, 4):
        if (rows * (k_int + 4) + w * 64 * ld) * 4 <= lds_max:
            return w
    return 0
