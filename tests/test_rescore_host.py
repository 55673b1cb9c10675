"""The host side of tests/test_rescore.py (no GPU): the reference of tests/_rescore_ref.py is right, its cases exercise what the
GPU test says they do, and the pair layout is pinned on an example written out by hand."""
import os

import numpy as np
import pytest

from tests import _rescore_ref as ref

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _source():
    with open(os.path.join(ROOT, "emgraph_amd", "csrc", "emg_rank.hip")) as f:
        return f.read()


def test_model_and_link_ids_are_the_librarys():
    from emgraph_amd import _lib as L
    assert [ref.MODELS[m] for m in ("TransE_L1", "TransE_L2", "DistMult", "ComplEx", "HolE")] == \
        [L.TRANSE_L1, L.TRANSE_L2, L.DISTMULT, L.COMPLEX, L.HOLE]
    assert [L.LINK_IDS[n] for n in ref.LINKS] == [0, 1, 2, 3]


# ---- 1. the reference is right ---------------------------------------------------------------------------------------------------
def _float64_scores(model, q, E, scale):
    q, E = q.astype(np.float64), E.astype(np.float64)
    if model == ref.TRANSE_L1:
        return -np.abs(q - E).sum(1)
    if model == ref.TRANSE_L2:
        return -np.sqrt(((q - E) ** 2).sum(1))
    if model == ref.HOLE:
        return (E @ q) * np.float64(F32(scale))
    return E @ q


@pytest.mark.parametrize("model_name", sorted(ref.MODELS))
def test_expected_equals_float64_on_small_integer_tables(model_name):
    """entries in -3..3, k_int = 36: every difference, product and partial sum is an integer below 2^24, so the float32 chain is exact
    in any order and a float64 restatement rounded once to float32 must give the same comparison integers, pair for pair"""
    case = ref.segment_case(model_name, 36)
    rs = np.random.RandomState(5)
    c = ref.SimpleNamespace(**vars(case))
    c.E = rs.randint(-3, 4, case.E.shape).astype(F32)
    c.Q = rs.randint(-3, 4, case.Q.shape).astype(F32)
    c.E[7], c.E[150] = c.E[3], c.E[100]
    c.pos_int = case.pos_int.copy()
    for r in range(c.n_rows - 1):
        c.pos_int[r] = ref.cmp_int(_float64_scores(c.model, c.Q[r], c.E[[3, 100, r % 200][r % 3]][None], c.scale).astype(F32))[0]
    gt, eq = ref.expected(c)
    want_gt, want_eq = np.zeros_like(gt), np.zeros_like(eq)
    for rows, ents in ref.counted(c):
        for r, e in zip(rows, ents):
            ci = int(ref.cmp_int(_float64_scores(c.model, c.Q[r], c.E[e][None], c.scale).astype(F32))[0])
            want_gt[r] += ci > c.pos_int[r]
            want_eq[r] += ci == c.pos_int[r]
    assert np.array_equal(gt, want_gt) and np.array_equal(eq, want_eq)
    assert (gt > 0).sum() >= 20 and (eq > 0).sum() >= 10 and gt[c.sentinel] == 0 and eq[c.sentinel] == 0


def test_expected_reads_no_entry_behind_a_count():
    """padding entries moved to a counted row and another entity change nothing; the overflowed segment is read to cap"""
    case = ref.segment_case("DistMult", 20)
    gt, eq = ref.expected(case)
    c = ref.SimpleNamespace(**vars(case))
    c.pairs = case.pairs.copy()
    for s in range(c.n_seg):
        c.pairs[s, min(int(c.pair_count[s]), c.cap):] = (np.int64(5) << 32) | 9
    gt2, eq2 = ref.expected(c)
    assert np.array_equal(gt, gt2) and np.array_equal(eq, eq2)
    s = int(np.flatnonzero(case.pair_count[:case.n_seg] == ref.CAP + 5)[0])
    assert len(ref.counted(case)[s][0]) == ref.CAP
    assert sum(len(x[0]) for x in ref.counted(case)) == sum(min(n, ref.CAP) for n, _, _ in ref.SEGMENTS)


# ---- 2. the cases are not vacuous --------------------------------------------------------------------------------------------------
def _gpu_cases():
    """every case tests/test_rescore.py runs: (id, case, long-segment threshold of the LDS form at its width, linear)"""
    limits = ref.lds_limits(_source())
    out = []
    for m in sorted(ref.MODELS):
        for k in ref.WIDTHS + (37,):
            waves = ref.image_waves(k, limits) if k % 4 == 0 else 0
            out.append(("%s-%d" % (m, k), m, k, "linear", limits[3] // (1 if waves != 4 else 2)))
    for m in ref.LINK_MODELS:
        for k in ref.LINK_WIDTHS:
            for link in ref.LINKS[1:]:
                out.append(("%s-%d-%s" % (m, k, link), m, k, link, limits[3] // (1 if ref.image_waves(k, limits) != 4 else 2)))
    return out


@pytest.mark.parametrize("cid,model_name,k_int,link,min_long", _gpu_cases(), ids=[c[0] for c in _gpu_cases()])
def test_case_exercises_every_form(cid, model_name, k_int, link, min_long):
    case = ref.segment_case(model_name, k_int, link)
    assert case.Q.shape == (130, k_int) and case.E.shape == (200, k_int) and case.pairs.shape == (27, 1600)
    assert case.pairs.dtype == np.int64 and case.pair_count.shape == (28,) and case.sentinel == 129
    cov = ref.coverage(case)        # against the 512-pair threshold, whatever the width
    assert cov["below_256"] >= 3 and cov["from_256_below_512"] >= 3 and cov["from_512"] >= 3
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, ref.CAP, ref.CAP + 5):
        assert n in cov["sizes"], n
    assert cov["truncated"]
    assert all(cov["spans"][k] >= 2 for k in ref.SPANS), cov["spans"]
    assert all(cov["orders"][k] >= 2 for k in ref.ORDERS), cov["orders"]
    assert cov["wraps"] >= 4 and cov["staged"] >= 4 and cov["unstaged"] >= 4
    assert cov["duplicates"] >= 50
    assert cov["sentinel_counted"] == 0 and cov["sentinel_padding"] and cov["in_range"]
    if link == "linear":
        assert cov["rows_gt"] >= 20 and cov["rows_eq"] >= 10, (cov["rows_gt"], cov["rows_eq"])
    # what the builders say they built is what the buffers hold
    for s, (rows, ents) in enumerate(ref.counted(case)):
        if len(rows) >= 512:
            assert ref.span_kind(rows) == case.seg_kind[s] and ref.entity_order(ents) == case.seg_order[s]
    if min_long != 512:             # the 4-wave image: its threshold is lower, the same holds there
        cov = ref.coverage(case, min_long)
        assert cov["long"] > ref.coverage(case)["long"] and cov["staged"] >= 4 and cov["unstaged"] >= 4
    # an offset slab: the same pairs, global ids
    off = ref.with_offset(case, 1000)
    assert np.array_equal(off.pairs - case.pairs, np.full_like(case.pairs, 1000)) and ref.coverage(off)["in_range"]
    ptr, idx = ref.as_csr(off)
    assert ptr[-1] == len(idx) == sum(len(x[0]) for x in ref.counted(case)) and ptr[129] == ptr[130] and idx.min() >= 1000


def test_big_tile_case():
    case = ref.big_tile_case()
    assert case.E.shape == (ref.BIG_N_LOCAL, 4) and case.E.nbytes > 4 << 20
    n_tiles = -(-ref.BIG_N_LOCAL // 32)
    assert n_tiles > 8192 and ref.BIG_N_LOCAL % 32 == 8 and ref.BIG_TILES[-1] == n_tiles - 1
    segs = ref.counted(case)
    tiles = np.concatenate([s[1] for s in segs]) // 32
    for t in ref.BIG_TILES:
        assert (tiles == t).sum() >= 100, t
    assert set(np.unique(tiles)) == set(ref.BIG_TILES)
    cov = ref.coverage(case)
    assert cov["in_range"] and cov["sentinel_counted"] == 0 and cov["sentinel_padding"] and cov["duplicates"] >= 10
    assert cov["rows_gt"] >= 20 and cov["rows_eq"] >= 10


def test_widths_straddle_the_image_limits():
    """572 | 576: the last width of the 8-wave image and the first of the 4-wave one; 860 | 864: the last width any image fits"""
    limits = ref.lds_limits(_source())
    assert limits[0] == ref.RQ_ROWS and limits[3] == 512
    assert [ref.image_waves(k, limits) for k in (572, 576, 860, 864)] == [8, 4, 4, 0]
    assert [ref.image_waves(k, limits) for k in ref.WIDTHS] == [8, 8, 8, 8, 8, 8, 8, 4, 0]
    assert all(ref.image_waves(k, limits) for k in ref.TILE_WIDTHS)


# ---- 3. the packing, by hand ---------------------------------------------------------------------------------------------------------
def test_packing_and_clamp_by_hand():
    """three segments of capacity 4 over a slab that starts at global entity 1000; the third holds a count above its capacity"""
    sent = 5
    pairs = np.array([[(2 << 32) | 1003, (0 << 32) | 1000, (sent << 32) | 1001, (sent << 32) | 1001],
                      [(sent << 32) | 1002, (sent << 32) | 1002, (sent << 32) | 1002, (sent << 32) | 1002],
                      [(4 << 32) | 1001, (4 << 32) | 1001, (1 << 32) | 1004, (3 << 32) | 1002]], np.int64)
    E = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [1, 1, 0, 0]], F32)
    Q = np.array([[2, 0, 0, 0], [1, 1, 0, 0], [0, 0, 0, 3], [0, 0, 1, 0], [0, 5, 0, 0], [9, 9, 9, 9]], F32)
    case = ref.SimpleNamespace(model=ref.DISTMULT, k_int=4, scale=1.0, link="linear", E=E, Q=Q,
                               pos_int=np.array([100000, 200000, 300000, 100000, 0, np.iinfo(np.int32).min], np.int32),
                               pairs=pairs, pair_count=np.array([2, 0, 9, 0], np.int32), ent_offset=1000, cap=4, n_seg=3, n_rows=6,
                               sentinel=sent)
    segs = ref.counted(case)
    assert [list(map(int, s[0])) for s in segs] == [[2, 0], [], [4, 4, 1, 3]]
    assert [list(map(int, s[1])) for s in segs] == [[3, 0], [], [1, 1, 4, 2]]
    gt, eq = ref.expected(case)
    # scores: (2,3) = 3, (0,0) = 2, (4,1) = 5 twice, (1,4) = 2, (3,2) = 1
    assert list(gt) == [1, 0, 0, 0, 2, 0] and list(eq) == [0, 1, 1, 1, 0, 0]
    ptr, idx = ref.as_csr(case)
    assert list(ptr) == [0, 1, 2, 3, 4, 6, 6] and list(idx) == [1000, 1004, 1003, 1002, 1001, 1001]
    assert int(pairs[0, 0]) == 2 * 2 ** 32 + 1003 and int(pairs[0, 0]) >> 32 == 2 and int(pairs[0, 0]) & 0xffffffff == 1003
