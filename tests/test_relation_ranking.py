"""Relation prediction on the GPU: rank and complete (s, ?, o) against the relation table (csrc/emg_relrank.hip).

Every expected value comes from OUTSIDE the new code.  One triple, one score: the relation-side score of (s_i, r, o_i) is the
object-side one, so the expected dense scores are device.eval_build_queries(..., EVAL_O) + device.eval_scores_dense on the
expanded triples (s_i, r, o_i), column o_i, and the expected pos_int is the second return value of eval_build_queries on the
test triples.  Score bits, counters and ids must be EQUAL, not close.  Counters and the total order are formed on the host
(tests/_relrank_ref.py) from those scores."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from emgraph_amd import _lib as L  # noqa: E402
from tests import _chain_ref as chain  # noqa: E402
from tests import _relrank_ref as ref  # noqa: E402

F32 = np.float32
NMAX = L.TOPN_MAX
MODELS = {"DistMult": (L.DISTMULT, None), "ComplEx": (L.COMPLEX, None), "HolE": (L.HOLE, None), "RotatE": (L.ROTATE, None),
          "TransE_L1": (L.TRANSE_L1, None), "TransE_L2": (L.TRANSE_L2, None), "TransE_3": (L.TRANSE_P, 3.0)}
CPLX = ("ComplEx", "HolE", "RotatE")
N_ENT = 100


def dev():
    from emgraph_amd import device
    device.require_gpu()
    return device


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def table(a):
    """a device table as the package holds it (rows padded to the library's stride, 16-byte aligned)"""
    from emgraph_amd.training import alloc_table
    a = np.ascontiguousarray(a, dtype=F32)
    return alloc_table(a.shape[0], a.shape[1], torch.device("cuda"), init=a)


def kint_scale(name, k):
    ki = 2 * k if name in CPLX else k
    return ki, MODELS[name][1] or (float(F32(2 / k)) if name == "HolE" else 1.0)


def make_tables(name, k, n_rel, seed, n_ent=N_ENT):
    ki, _ = kint_scale(name, k)
    rs = np.random.RandomState(seed)
    E = (rs.randn(n_ent, ki) * 0.3).astype(F32)
    R = (rs.randn(n_rel, ki) * 0.3).astype(F32)
    if name == "RotatE":   # phases in the first k columns, the rest unused and zero
        R[:, :k] = rs.uniform(-np.pi, np.pi, (n_rel, k))
        R[:, k:] = 0
    return E, R


def triples(n_ent, n_rel, rows, seed):
    rs = np.random.RandomState(seed)
    return np.stack([rs.randint(0, n_ent, rows), rs.randint(0, n_rel, rows), rs.randint(0, n_ent, rows)], 1).astype(np.int32)


def expected(mid, ent, rel, ki, scale, T, cands, link=L.LINK_LINEAR, want_q=False):
    """(dense scores f32 [rows, n_cand], pos_int int32 [rows]) by the OBJECT-SIDE kernels that were here before"""
    d = dev()
    X = ref.expand(T[:, 0], T[:, 2], cands)
    Q, _ = d.eval_build_queries(mid, ent, rel, ki, scale, cu(X), L.EVAL_O)
    objs = np.unique(T[:, 2].astype(np.int64))
    S_all = d.eval_scores_dense(mid, Q, ent, ki, scale, cand=cu(objs.astype(np.int32))).cpu().numpy()
    _, pos = d.eval_build_queries(mid, ent, rel, ki, scale, cu(T), L.EVAL_O, link=link)
    S = ref.pick_objects(S_all, T[:, 2], len(cands), objs)
    return (S, pos, Q) if want_q else (S, pos)


def rel_operand(mid, rel, ki):
    return dev().eval_rel_rotate_image(rel, ki) if mid == L.ROTATE else rel


def csr(excl, rows):
    ptr = np.zeros(rows + 1, np.int64)
    ptr[1:] = np.cumsum([len(e) for e in excl])
    idx = np.concatenate([np.sort(np.asarray(e, np.int32)) for e in excl] + [np.zeros(0, np.int32)])
    return cu(ptr), cu(idx.astype(np.int32))


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


def check_all(name, ent, rel, k, T, seed, cands=None, top_ns=(1, 10, NMAX)):
    """dense scores, the four counters (random exclusion lists that hold the positive) and the top-N of every size against
    the object-side expectation; returns the expected scores"""
    d = dev()
    mid = MODELS[name][0]
    ki, scale = kint_scale(name, k)
    n_rel, rows = rel.shape[0], len(T)
    cand_ids = np.arange(n_rel) if cands is None else np.asarray(cands)
    candt = None if cands is None else cu(cand_ids.astype(np.int32))
    S_want, pos = expected(mid, ent, rel, ki, scale, T, cand_ids)
    op = rel_operand(mid, rel, ki)
    Tt = cu(T)
    S_got = d.eval_rel_scores_dense(mid, ent, op, ki, scale, Tt, cand_rel=candt)
    assert S_got.shape == (rows, len(cand_ids))
    assert np.array_equal(bits(S_got.cpu().numpy()), bits(S_want)), np.argwhere(bits(S_got.cpu().numpy()) != bits(S_want))[:5]
    # the same triple's pos_int, object side against relation side
    C = ref.cmp_int(S_want)
    pos_h = pos.cpu().numpy()
    if cands is None:
        assert np.array_equal(C[np.arange(rows), T[:, 1]], pos_h)
    rs = np.random.RandomState(seed)
    excl = [sorted(set(rs.choice(n_rel, rs.randint(0, min(n_rel, 6) + 1), replace=False).tolist()) | {int(p)}) for p in T[:, 1]]
    ptr, idx = csr(excl, rows)
    cnt = d.eval_rel_count(mid, ent, op, ki, scale, Tt, pos, cand_rel=candt, excl_ptr=ptr, excl_idx=idx).cpu().numpy()
    want = ref.counts(C, pos_h, cand_ids, excl)
    for got, w, what in zip(cnt, want, ("cnt_gt", "cnt_eq", "fcnt_gt", "fcnt_eq")):
        assert np.array_equal(got, w), (what, np.argwhere(got != w)[:5])
    known = [e[:-1] if len(e) > 1 else [] for e in excl]
    ptr, idx = csr(known, rows)
    for top_n in top_ns:
        want_i, want_s = ref.host_topn(S_want, cand_ids, top_n, known)
        got_i, got_s = d.eval_rel_topn(S_got, top_n, cand_rel=candt, excl_ptr=ptr, excl_idx=idx)
        got_i, got_s = got_i.cpu().numpy(), bits(got_s.cpu().numpy())
        assert got_i.shape == (rows, top_n)
        assert np.array_equal(got_i, want_i), (top_n, np.argwhere(got_i != want_i)[:5])
        assert np.array_equal(got_s, want_s), (top_n, np.argwhere(got_s != want_s)[:5])
    return S_want


# (k, n_rel, rows): k-slice tails (3, 50), a single relation, relation counts that are no multiple of a tile (5 of 16; 67 and 300 of
# 64: the wide form), several relation tiles (67, 300), partial workgroups (1, 33 rows), several workgroups of the wide form's 64 pairs
# (130 rows); top_n above n_rel pads
SWEEP = [(3, 1, 1), (50, 5, 33), (200, 67, 130), (3, 300, 33), (50, 300, 130), (200, 5, 1)]


@pytest.mark.parametrize("name", sorted(MODELS))
@pytest.mark.parametrize("k,n_rel,rows", SWEEP)
def test_sweep_matches_the_object_side(name, k, n_rel, rows):
    E, R = make_tables(name, k, n_rel, seed=k + n_rel)
    T = triples(N_ENT, n_rel, rows, seed=rows)
    check_all(name, table(E), table(R), k, T, seed=k)


@pytest.mark.parametrize("n_rel", [47, 48, 49, 64, 65])
def test_either_side_of_the_wide_form(n_rel):
    """from 48 candidates on the kernel maps four lanes to a pair and walks tiles of 64 relations: the sizes around the switch and
    around one whole tile, 70 rows (a partial workgroup of either form)"""
    for name, k in (("ComplEx", 6), ("TransE_L2", 9), ("RotatE", 5)):
        E, R = make_tables(name, k, n_rel, seed=n_rel)
        check_all(name, table(E), table(R), k, triples(N_ENT, n_rel, 70, seed=n_rel + 1), seed=3, top_ns=(10,))
    # a candidate list of 50 out of 65: the wide form reads its ids from the list
    if n_rel == 65:
        E, R = make_tables("DistMult", 7, n_rel, seed=1)
        cands = np.sort(np.random.RandomState(2).choice(n_rel, 50, replace=False))
        check_all("DistMult", table(E), table(R), 7, triples(N_ENT, n_rel, 70, seed=4), seed=5, cands=cands, top_ns=(10,))


def test_more_than_one_workgroup_of_rows():
    """600 rows against 21 relations: three workgroups of 256 pairs (the narrow form), the last one partial"""
    E, R = make_tables("ComplEx", 6, 21, seed=2)
    check_all("ComplEx", table(E), table(R), 6, triples(N_ENT, 21, 600, seed=3), seed=1, top_ns=(10,))
    E, R = make_tables("TransE_L1", 9, 21, seed=2)
    check_all("TransE_L1", table(E), table(R), 9, triples(N_ENT, 21, 600, seed=3), seed=1, top_ns=(10,))


@pytest.mark.parametrize("name", ["ComplEx", "HolE"])
def test_chain_order_on_mixed_tables(name):
    """tables whose every seventh column is 1000 times the others (tests/_chain_ref.mixed): a chain run in another order —
    re and im interleaved, say — rounds differently and changes the bits.  Both tables times 2^-6 (exact: the roundings
    stay where they were) so that score * 1e5 stays inside the int32 range of the comparison integer."""
    k = 25
    E, R = chain.mixed(N_ENT, 2 * k, seed=1) * F32(2.0 ** -6), chain.mixed(21, 2 * k, seed=2) * F32(2.0 ** -6)
    check_all(name, table(E), table(R), k, triples(N_ENT, 21, 40, seed=5), seed=2, top_ns=(10,))


@pytest.mark.parametrize("name", ref.ORACLE_MODELS + ("RotatE",))
def test_host_oracle_gives_the_same_bits(name):
    """the C oracle's object-side queries and chain (RotatE: the numpy float32 chain on device-built query rows)"""
    d = dev()
    k, n_rel, rows = 10, 21, 33
    mid = MODELS[name][0]
    ki, scale = kint_scale(name, k)
    E, R = make_tables(name, k, n_rel, seed=4)
    T = triples(N_ENT, n_rel, rows, seed=6)
    ent, rel = table(E), table(R)
    got = d.eval_rel_scores_dense(mid, ent, rel_operand(mid, rel, ki), ki, scale, cu(T)).cpu().numpy()
    if name == "RotatE":
        _, _, Q = expected(mid, ent, rel, ki, scale, T, np.arange(n_rel), want_q=True)
        want = ref.rotate_scores(Q.cpu().numpy()[:, :ki], E, T[:, 2], n_rel)
    else:
        want = ref.scores(name, E, R, ki, scale, T[:, 0], T[:, 2], np.arange(n_rel))
    assert np.array_equal(bits(got), bits(want))


def test_ties_all_zero_relation_table():
    d = dev()
    for name in ("DistMult", "TransE_L1", "ComplEx"):
        k, n_rel, rows = 8, 40, 33
        ki, scale = kint_scale(name, k)
        E, _ = make_tables(name, k, n_rel, seed=1)
        ent, rel = table(E), table(np.zeros((n_rel, ki), F32))
        T = triples(N_ENT, n_rel, rows, seed=2)
        S = check_all(name, ent, rel, k, T, seed=3)
        assert (bits(S) == bits(S[:, :1])).all()   # every relation ties
        ids, _ = d.eval_rel_topn(cu(S), 10)
        assert np.array_equal(ids.cpu().numpy(), np.tile(np.arange(10, dtype=np.int32), (rows, 1)))
        _, pos = expected(MODELS[name][0], ent, rel, ki, scale, T, np.arange(n_rel))
        cnt = d.eval_rel_count(MODELS[name][0], ent, rel, ki, scale, cu(T), pos).cpu().numpy()
        assert (cnt[0] == 0).all() and (cnt[1] == n_rel).all() and (cnt[2:] == 0).all()


def test_ties_identical_relation_rows_in_different_tiles():
    d = dev()
    for name in ("DistMult", "ComplEx", "TransE_L2", "RotatE"):
        k, n_rel, rows = 8, 40, 33
        E, R = make_tables(name, k, n_rel, seed=5)
        R[20] = R[3]   # tiles 1 and 0 of 16 relations
        R[37] = R[3]
        S = check_all(name, table(E), table(R), k, triples(N_ENT, n_rel, rows, seed=7), seed=4)
        assert np.array_equal(bits(S[:, 3]), bits(S[:, 20])) and np.array_equal(bits(S[:, 3]), bits(S[:, 37]))
        ids = d.eval_rel_topn(cu(S), n_rel)[0].cpu().numpy()
        for r in range(rows):
            p = int(np.flatnonzero(ids[r] == 3)[0])
            assert ids[r, p:p + 3].tolist() == [3, 20, 37]


def test_total_order_on_hand_made_scores():
    """-0 == +0, NaN last, equal scores by ascending id, padding (-1, -inf); and TransE-L1's own -0 scores"""
    d = dev()
    row = np.array([0.0, -0.0, np.nan, 1.0, -np.inf, np.inf, -0.0, 0.0], F32)
    S = np.stack([row, row[::-1].copy()])
    for top_n in (1, 5, 8, 10, NMAX):
        want_i, want_s = ref.host_topn(S, np.arange(8), top_n)
        got_i, got_s = d.eval_rel_topn(cu(S), top_n)
        assert np.array_equal(got_i.cpu().numpy(), want_i) and np.array_equal(bits(got_s.cpu().numpy()), want_s)
    got_i, got_s = d.eval_rel_topn(cu(S), 10)
    got_i, got_s = got_i.cpu().numpy(), got_s.cpu().numpy()
    assert got_i[0].tolist() == [5, 3, 0, 1, 6, 7, 4, 2, -1, -1]
    assert np.isnan(got_s[0, 7]) and np.isneginf(got_s[0, 8:]).all() and np.signbit(got_s[0, 3]) and not np.signbit(got_s[0, 2])
    # a candidate list names the ids; an excluded winner takes no slot
    cand = np.array([2, 3, 5, 7, 11, 13, 17, 19], np.int32)
    ptr, idx = csr([[13, 3], []], 2)
    want_i, want_s = ref.host_topn(S, cand, 10, [[3, 13], []])
    got_i, got_s = d.eval_rel_topn(cu(S), 10, cand_rel=cu(cand), excl_ptr=ptr, excl_idx=idx)
    assert np.array_equal(got_i.cpu().numpy(), want_i) and np.array_equal(bits(got_s.cpu().numpy()), want_s)
    # s + r - o = 0 in every coordinate: TransE-L1 scores -0 for the zero relations, below it for the others
    E = np.zeros((N_ENT, 8), F32)
    R = np.zeros((20, 8), F32)
    R[1::2] = 0.25
    T = triples(N_ENT, 20, 5, seed=1)
    Sz = check_all("TransE_L1", table(E), table(R), 8, T, seed=1)
    assert (bits(Sz[:, ::2]) == np.int32(-2 ** 31)).all() and (Sz[:, 1::2] == -2.0).all()
    ids = d.eval_rel_topn(cu(Sz), 20)[0].cpu().numpy()
    assert ids[0].tolist() == list(range(0, 20, 2)) + list(range(1, 20, 2))


def test_no_rows_and_no_candidates():
    d = dev()
    E, R = make_tables("DistMult", 8, 5, seed=1)
    ent, rel = table(E), table(R)
    T = triples(N_ENT, 5, 3, seed=1)
    assert d.eval_rel_scores_dense(L.DISTMULT, ent, rel, 8, 1.0, cu(T[:0])).shape == (0, 5)
    none = cu(np.zeros(0, np.int32))
    cnt = d.eval_rel_count(L.DISTMULT, ent, rel, 8, 1.0, cu(T), cu(np.zeros(3, np.int32)), cand_rel=none)
    assert (cnt.cpu().numpy() == 0).all()
    S = d.eval_rel_scores_dense(L.DISTMULT, ent, rel, 8, 1.0, cu(T), cand_rel=none)
    ids, sc = d.eval_rel_topn(S, 4, cand_rel=none)
    assert (ids.cpu().numpy() == -1).all() and np.isneginf(sc.cpu().numpy()).all()
    for bad in (0, NMAX + 1):
        with pytest.raises(L.EmgError, match="top_n"):
            d.eval_rel_topn(cu(np.zeros((2, 3), F32)), bad)


@pytest.mark.parametrize("name", ["DistMult", "TransE_L1"])
def test_unaligned_rows_take_the_scalar_loads(name):
    """tables whose rows are not 16-byte aligned (stride 7)"""
    rs = np.random.RandomState(3)
    ent = cu((rs.randn(N_ENT, 7) * 0.3).astype(F32))
    rel = cu((rs.randn(21, 7) * 0.3).astype(F32))
    assert ent.stride(0) == 7 and rel.stride(0) == 7
    check_all(name, ent, rel, 7, triples(N_ENT, 21, 70, seed=4), seed=5, top_ns=(10,))


# ------------------------------------------------------------------------------------------------ filter, subset, strategies
def coarse_tables(name, k, n_rel, seed):
    """quarter-integer tables: many equal scores, so the three strategies differ"""
    ki, _ = kint_scale(name, k)
    rs = np.random.RandomState(seed)
    return rs.randint(-2, 3, (N_ENT, ki)).astype(F32) / 4, rs.randint(-2, 3, (n_rel, ki)).astype(F32) / 4


@pytest.mark.parametrize("name", ["DistMult", "ComplEx", "TransE_L1"])
def test_filter_subset_and_the_three_strategies(name):
    from emgraph_amd.evaluation.ranking import FilterIndex, rank_relations_device, topn_relations_device
    mid = MODELS[name][0]
    k, n_rel, rows = 3, 21, 40
    ki, scale = kint_scale(name, k)
    E, R = coarse_tables(name, k, n_rel, seed=8)
    ent, rel = table(E), table(R)
    T = triples(N_ENT, n_rel, rows, seed=9)
    T[1, [0, 2]] = T[0, [0, 2]]   # rows 0 and 1: the same pair
    # known relations: row 0's pair holds every relation (full), rows 2.. a few others, row 5's nothing but its positive
    Fl = [(T[0, 0], p, T[0, 2]) for p in range(n_rel)]
    rs = np.random.RandomState(10)
    for r in range(2, rows):
        if r != 5:
            Fl += [(T[r, 0], int(p), T[r, 2]) for p in rs.choice(n_rel, 4, replace=False)]
    Fl += [tuple(T[5]), tuple(T[5])]   # a duplicated filter triple
    Farr = np.array(Fl, np.int64)
    known = [sorted({int(p) for s, p, o in Farr if s == T[r, 0] and o == T[r, 2]}) for r in range(rows)]
    S, pos = expected(mid, ent, rel, ki, scale, T, np.arange(n_rel))
    C, pos_h = ref.cmp_int(S), pos.cpu().numpy()
    some_tie = False
    for subset in (None, np.array([20, 1, 4, 4, 9, 16, 17])):     # (unsorted, a repeat: the candidates are its distinct ids)
        cand_ids = np.arange(n_rel) if subset is None else np.unique(subset)
        if subset is not None:
            assert (~np.isin(T[:, 1], cand_ids)).any()             # rows whose positive is no candidate
        for F in (None, Farr):
            excl = None
            if F is not None:
                excl = [sorted((set(known[r]) & set(cand_ids.tolist())) | {int(T[r, 1])}) for r in range(rows)]
            gt, eq, fgt, feq = ref.counts(C[:, cand_ids], pos_h, cand_ids, excl)
            some_tie |= bool((eq > 1).any())
            for strategy in ("worst", "best", "middle"):
                got = rank_relations_device(mid, ent, rel, ki, scale, T, strategy, filter_triples=F, relations_subset=subset,
                                            query_chunk=16)
                assert got.dtype == np.int64 and np.array_equal(got, ref.ranks(gt, eq, fgt, feq, strategy)), (strategy, subset is None)
            if F is not None and subset is None:
                assert (ref.ranks(gt, eq, fgt, feq, "worst")[:2] == 1).all()   # every relation of the pair is known: rank 1
        # top-N: the known relations never come back; a pair whose every relation is known gets padding only
        want_i, want_s = ref.host_topn(S[:, cand_ids], cand_ids, 10, known)
        got_i, got_s = topn_relations_device(mid, ent, rel, ki, scale, T[:, [0, 2]], 10, filter_triples=FilterIndex(Farr),
                                             relations_subset=subset, query_chunk=16)
        assert np.array_equal(got_i, want_i) and np.array_equal(bits(got_s), want_s)
        assert (got_i[:2] == -1).all() and np.isneginf(got_s[:2]).all()
    assert some_tie
    # exclusion lists that are empty (a CSR of zeros) count nothing
    d = dev()
    ptr, idx = csr([[] for _ in range(rows)], rows)
    cnt = d.eval_rel_count(mid, ent, rel, ki, scale, cu(T), pos, excl_ptr=ptr, excl_idx=idx).cpu().numpy()
    want = ref.counts(C, pos_h, np.arange(n_rel), None)
    assert all(np.array_equal(a, b) for a, b in zip(cnt, want)) and (cnt[2:] == 0).all()
    assert rank_relations_device(mid, ent, rel, ki, scale, T[:0], "worst").shape == (0,)
    assert topn_relations_device(mid, ent, rel, ki, scale, T[:0, :2], 3)[0].shape == (0, 3)


# ------------------------------------------------------------------------------------------------ through a link
@pytest.mark.parametrize("name", ["DistMult", "TransE_L1", "RotatE"])
def test_counts_through_the_tanh_link(name):
    """the counters of the LINKED instantiation against host counts on the device's own link bits (emg_link_scores on the raw
    scores, the integer formed with float32 arithmetic), as tests/test_link_ranking.py takes them"""
    from emgraph_amd.evaluation.ranking import rank_relations_device
    d = dev()
    mid = MODELS[name][0]
    k, n_rel, rows = 10, 37, 70
    ki, scale = kint_scale(name, k)
    E, R = make_tables(name, k, n_rel, seed=12)
    E *= F32(0.5)   # raw scores of order one: the link is not saturated
    ent, rel = table(E), table(R)
    T = triples(N_ENT, n_rel, rows, seed=13)
    S, pos = expected(mid, ent, rel, ki, scale, T, np.arange(n_rel), link=L.LINK_TANH)
    lin = cu(S.reshape(-1).copy())
    d.link_scores(L.LINK_TANH, None, 0.0, lin[:rows].clone(), lin, rows, n_rel)   # in place: weight 1 * phi(score)
    C = ref.cmp_int(lin.cpu().numpy().reshape(rows, n_rel))
    pos_h = pos.cpu().numpy()
    assert np.array_equal(C[np.arange(rows), T[:, 1]], pos_h)
    excl = [[int(p)] for p in T[:, 1]]
    ptr, idx = csr(excl, rows)
    cnt = d.eval_rel_count(mid, ent, rel_operand(mid, rel, ki), ki, scale, cu(T), pos, excl_ptr=ptr, excl_idx=idx,
                           link=L.LINK_TANH).cpu().numpy()
    want = ref.counts(C, pos_h, np.arange(n_rel), excl)
    for got, w in zip(cnt, want):
        assert np.array_equal(got, w)
    got = rank_relations_device(mid, ent, rel, ki, scale, T, "worst", filter_triples=T, link=L.LINK_TANH)
    assert np.array_equal(got, ref.ranks(*want, "worst"))


# ------------------------------------------------------------------------------------------------ the public functions
def toy_graph(n_ent=40, n_rel=6, n=240, seed=0):
    rs = np.random.RandomState(seed)
    X = np.stack([rs.randint(0, n_ent, n), rs.randint(0, n_rel, n), rs.randint(0, n_ent, n)], 1)
    X[:n_ent, 0] = np.arange(n_ent)   # every entity and relation occurs
    X[:n_ent, 2] = np.arange(n_ent)[::-1]
    X[:n_rel, 1] = np.arange(n_rel)
    return np.array([["e%02d" % s, "r%d" % p, "e%02d" % o] for s, p, o in X])


@functools.lru_cache(maxsize=None)
def fitted(name, link="linear", through=False):
    from emgraph_amd import models
    params = {"non_linearity": link}
    if through:
        params["rank_through_link"] = True
    m = getattr(models, name)(k=5, epochs=2, batches_count=2, seed=3, embedding_model_params=params)
    m.fit(toy_graph())
    return m


def predict_tol(name, m, trip_idx, pred):
    """the tolerance tests/test_topn.py uses for "the returned scores are predict's": score_tol of tests/test_hip_kernels.py,
    1e-4 of the sum of the magnitudes of the terms the score sums, + 1e-7.  RotatE's score sums the k moduli |s_j r_j - o_j|,
    whose magnitudes add up to |score| itself: the same rule gives 1e-4 |score| + 1e-7."""
    from tests.test_hip_kernels import score_tol
    if name == "RotatE":
        return 1e-4 * np.abs(pred) + 1e-7
    E, R = (np.asarray(t, F32) for t in m.trained_model_params)
    return score_tol(name, E, R, trip_idx, 5)


@pytest.mark.parametrize("name,link", [("ComplEx", "linear"), ("RotatE", "linear"), ("ComplEx", "tanh")])
def test_public_api(name, link):
    from emgraph_amd.evaluation import (evaluate_relation_prediction, hits_at_n_score, mrr_score, to_idx, topn_relations)
    X = toy_graph()
    m = fitted(name, link, through=link != "linear")
    n_rel = len(m.rel_to_idx)
    Xi = to_idx(X, m.ent_to_idx, m.rel_to_idx)
    # ranks: the public function against the model's method on ids
    for strategy in ("worst", "best"):
        ranks = evaluate_relation_prediction(X[:60], m, filter_triples=X, ranking_strategy=strategy)
        assert ranks.shape == (60,) and ranks.dtype == np.int64 and ranks.min() >= 1 and ranks.max() <= n_rel
        assert np.array_equal(ranks, m.get_relation_ranks_idx(Xi[:60], filter_idx=Xi, ranking_strategy=strategy))
    assert 0 < mrr_score(ranks) <= 1 and 0 <= hits_at_n_score(ranks, 3) <= 1
    unseen = np.concatenate([X[:4], np.array([["nobody", "r0", "e01"]])])
    assert len(evaluate_relation_prediction(unseen, m)) == 4          # filter_unseen drops the fifth
    sub = evaluate_relation_prediction(X[:60], m, relations_subset=["r1", "r3", "r4"])
    assert sub.max() <= 4                                             # unfiltered: the positive's own tie counts, as on the entity sides
    # top-N: unfiltered with top_n = n_rel, every pair lists all the relations; the scores are predict's
    pairs = X[:30][:, [0, 2]]
    labels, scores = topn_relations(pairs, m, top_n=n_rel)
    assert labels.shape == (30, n_rel) and scores.shape == (30, n_rel) and scores.dtype == np.float32
    assert all(sorted(row) == sorted(m.rel_to_idx) for row in labels.tolist())
    assert np.all(np.diff(scores, axis=1) <= 0)
    ids, scores_i = topn_relations(Xi[:30][:, [0, 2]], m, top_n=n_rel, from_idx=True)
    assert np.array_equal(np.vectorize(m.rel_to_idx.get)(labels), ids) and np.array_equal(scores, scores_i)
    trip = np.stack([np.repeat(pairs[:, 0], n_rel), labels.reshape(-1), np.repeat(pairs[:, 1], n_rel)], 1)
    pred = m.predict(trip)
    tol = predict_tol(name, m, to_idx(trip, m.ent_to_idx, m.rel_to_idx), pred)   # (the links are 1-Lipschitz)
    assert np.all(np.abs(pred - scores.reshape(-1)) <= tol), np.abs(pred - scores.reshape(-1)).max()
    # the positive's place in the unfiltered list lies between its best and its worst rank
    best = m.get_relation_ranks_idx(Xi[:30], ranking_strategy="best")
    worst = m.get_relation_ranks_idx(Xi[:30], ranking_strategy="worst")
    for r in range(30):
        p = int(np.flatnonzero(ids[r] == Xi[r, 1])[0])
        assert best[r] - 1 <= p <= worst[r] - 1, (r, p, best[r], worst[r])
    # the filter: the known relations of a pair never come back; short rows are padded with None / -inf
    labels, scores = topn_relations(pairs, m, top_n=n_rel + 2, filter_triples=X)
    for r in range(30):
        known = {p for s, p, o in X if s == pairs[r, 0] and o == pairs[r, 1]}
        row = labels[r].tolist()
        assert not known & set(row) and row.count(None) == 2 + len(known)
        assert np.isneginf(scores[r, n_rel - len(known):]).all()
    labels, _ = topn_relations(pairs[:3], m, top_n=2, relations_subset=["r2", "r5"])
    assert all(sorted(row) == ["r2", "r5"] for row in labels.tolist())


def test_a_link_without_the_key_is_refused_as_get_ranks_idx_refuses_it():
    from emgraph_amd.evaluation import evaluate_relation_prediction
    m = fitted("ComplEx", "tanh", False)
    X = toy_graph()
    with pytest.raises(NotImplementedError, match="rank_through_link"):
        evaluate_relation_prediction(X[:8], m, filter_triples=X)
