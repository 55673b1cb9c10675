"""Top-N completions on the GPU.  The expected result of every test is computed OUTSIDE the new code: the dense scores of
device.eval_scores_dense(precision 0) on the same Q and table (or the numpy oracle), ordered on the host by the contract's
total order (higher score first, -0 == +0, NaN last, ties by ascending entity id) with the exclusions removed.  Ids must be
equal and scores bit-equal; every case runs with the library's chunking and with ent_chunk = 256, so the merge runs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from emgraph_amd import _lib as L  # noqa: E402
from oracle import emgraph_oracle as orc  # noqa: E402

F32 = np.float32
NMAX = L.TOPN_MAX
MODELS = {"DistMult": (L.DISTMULT, None), "ComplEx": (L.COMPLEX, None), "HolE": (L.HOLE, None),
          "TransE_L1": (L.TRANSE_L1, None), "TransE_L2": (L.TRANSE_L2, None), "TransE_3": (L.TRANSE_P, 3.0)}
CHUNKS = (0, 256)


def dev():
    from emgraph_amd import device
    device.require_gpu()
    return device


def table(a):
    """a device table as the package holds it (rows padded to the library's stride)"""
    from emgraph_amd.training import alloc_table
    a = np.ascontiguousarray(a, dtype=F32)
    return alloc_table(a.shape[0], a.shape[1], torch.device("cuda"), init=a)


def kint_scale(name, k):
    ki = 2 * k if name in ("ComplEx", "HolE") else k
    scale = MODELS[name][1] or (float(F32(2 / k)) if name == "HolE" else 1.0)
    return ki, scale


def host_topn(S, ids, top_n, excl=None):
    """rule 2 on dense scores S [rows, n_cand] of the candidates `ids`: (ids int32 [rows, N], score bits int32 [rows, N])"""
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


def csr(excl, rows):
    ptr = np.zeros(rows + 1, np.int64)
    ptr[1:] = np.cumsum([len(e) for e in excl])
    idx = np.concatenate([np.sort(np.asarray(e, np.int32)) for e in excl]) if rows else np.zeros(0, np.int32)
    return torch.from_numpy(ptr).cuda(), torch.from_numpy(idx.astype(np.int32)).cuda()


def check(model_id, Q, ent, ki, scale, top_n, cand=None, excl=None, chunks=CHUNKS):
    """emg_eval_topn against the dense scores of the same Q and table, for each chunking; returns the ids"""
    d = dev()
    rows = Q.shape[0]
    candt = None if cand is None else torch.from_numpy(np.asarray(cand, np.int32)).cuda()
    n_cand = ent.shape[0] if cand is None else len(cand)
    if rows and n_cand:
        S = d.eval_scores_dense(model_id, Q, ent, ki, scale, cand=candt).cpu().numpy()
    else:
        S = np.zeros((rows, n_cand), F32)
    ids = np.arange(ent.shape[0]) if cand is None else np.asarray(cand)
    want_i, want_s = host_topn(S, ids, top_n, excl)
    ptr = idx = None
    if excl is not None:
        ptr, idx = csr(excl, rows)
    for ec in chunks:
        got_i, got_s = d.eval_topn(model_id, Q, ent, ki, scale, top_n, cand=candt, excl_ptr=ptr, excl_idx=idx, ent_chunk=ec)
        got_i, got_s = got_i.cpu().numpy(), got_s.cpu().numpy().view(np.int32)
        assert got_i.shape == (rows, top_n)
        assert np.array_equal(got_i, want_i), (ec, np.argwhere(got_i != want_i)[:5])
        assert np.array_equal(got_s, want_s), (ec, np.argwhere(got_s != want_s)[:5])
    return want_i


def queries(name, E, R, k, rows, seed, side=L.EVAL_O):
    d = dev()
    ki, scale = kint_scale(name, k)
    rs = np.random.RandomState(seed)
    n_ent, n_rel = E.shape[0], R.shape[0]
    spo = np.stack([rs.randint(0, n_ent, rows), rs.randint(0, n_rel, rows), rs.randint(0, n_ent, rows)], 1).astype(np.int32)
    ent, rel = (E if torch.is_tensor(E) else table(E)), table(R)
    Q, _ = d.eval_build_queries(MODELS[name][0], ent, rel, ki, scale, torch.from_numpy(spo).cuda(), side)
    return Q, ent, ki, scale, spo


def random_case(name, k, n_ent, rows, seed, side=L.EVAL_O):
    ki, _ = kint_scale(name, k)
    rs = np.random.RandomState(seed)
    E = (rs.randn(n_ent, ki) * 0.3).astype(F32)
    R = (rs.randn(5, ki) * 0.3).astype(F32)
    return queries(name, E, R, k, rows, seed + 1, side)


# (k, |E|, rows, top_n): every k, |E|, rows and top_n of the sweep appears, and the extremes meet (one row against 4099 entities
# with top_n 1, 130 rows = two row tiles against 4099 with EMG_TOPN_MAX, a table smaller than top_n)
SWEEP = [(3, 100, 1, 1), (50, 1000, 33, 10), (200, 4099, 130, NMAX), (3, 4099, 33, 10), (50, 100, 130, NMAX), (200, 1000, 1, 1)]


@pytest.mark.parametrize("name", sorted(MODELS))
@pytest.mark.parametrize("k,n_ent,rows,top_n", SWEEP)
def test_sweep_matches_dense_scores(name, k, n_ent, rows, top_n):
    Q, ent, ki, scale, _ = random_case(name, k, n_ent, rows, seed=k + n_ent)
    check(MODELS[name][0], Q, ent, ki, scale, top_n)


@pytest.mark.parametrize("name", ["DistMult", "TransE_L1"])
def test_unpadded_rows_take_the_scalar_loads(name):
    """tables whose rows are not 16-byte aligned (stride 7)"""
    dev()
    rs = np.random.RandomState(3)
    E = torch.from_numpy((rs.randn(700, 7) * 0.3).astype(F32)).cuda()
    Qh = torch.from_numpy((rs.randn(40, 7) * 0.3).astype(F32)).cuda()
    assert E.stride(0) == 7
    check(MODELS[name][0], Qh, E, 7, 1.0, 10)


def test_ties_all_zero_table():
    for name in ("DistMult", "TransE_L2"):
        Q, ent, ki, scale, _ = queries(name, np.zeros((1000, 8), F32), np.zeros((2, 8), F32), 8, 33, seed=1)
        for top_n in (1, 10, NMAX):
            want = check(MODELS[name][0], Q, ent, ki, scale, top_n)
            assert np.array_equal(want, np.tile(np.arange(top_n, dtype=np.int32), (33, 1)))


def test_ties_identical_blocks_across_chunks():
    """dyadic table, blocks of 96 identical entity rows (a block straddles the 256-candidate chunk boundary): equal scores in id order"""
    rs = np.random.RandomState(7)
    block = rs.randint(-4, 5, (11, 8)).astype(F32) / 8
    E = np.repeat(block, 96, axis=0)[:1000]
    R = rs.randint(-4, 5, (3, 8)).astype(F32) / 8
    for name in ("DistMult", "ComplEx", "TransE_L1"):
        k = 4 if name == "ComplEx" else 8
        Q, ent, ki, scale, _ = queries(name, E, R, k, 33, seed=2)
        for top_n in (10, NMAX):
            check(MODELS[name][0], Q, ent, ki, scale, top_n)


def test_negative_zero_ties_with_positive_zero():
    """DistMult queries with negative coordinates against entity rows of zeros of either sign: whatever signs of zero the chain
    produces, they tie and come back in id order, between the one positive and the one negative score"""
    d = dev()
    E = np.zeros((300, 4), F32)
    E[1::3, 1] = -0.0
    E[5] = [1, 0, 0, 0]
    E[6] = [-1, 0, 0, 0]
    Qh = np.array([[-1, 0, 0, 0], [-1, -1, -1, -1]], F32)
    Q, ent = table(Qh), table(E)
    S = d.eval_scores_dense(L.DISTMULT, Q, ent, 4, 1.0).cpu().numpy()
    assert S[0, 5] < 0 < S[0, 6] and not S[0, :5].any()
    want = check(L.DISTMULT, Q, ent, 4, 1.0, 10)
    assert want[0, 0] == 6 and want[1, 0] == 6 and list(want[0, 1:4]) == [0, 1, 2]
    got = check(L.DISTMULT, Q, ent, 4, 1.0, NMAX)
    assert 5 not in got[0].tolist()   # the negative score is the last of 300


@pytest.mark.parametrize("reverse", [False, True])
def test_worst_order_every_candidate_takes_the_rare_path(reverse):
    """entity i scores i * 2^-10 against a query of ones: increasing with the id (every candidate beats the running N-th best)"""
    n = 4099
    E = np.zeros((n, 8), F32)
    E[:, 0] = np.arange(n, dtype=F32) * F32(2.0 ** -10)
    if reverse:
        E = E[::-1].copy()
    Q, ent = table(np.ones((3, 8), F32)), table(E)
    for top_n in (1, 10, NMAX):
        want = check(L.DISTMULT, Q, ent, 8, 1.0, top_n)
        first = 0 if reverse else n - 1
        assert want[0, 0] == first


def test_short_rows_are_padded():
    Q, ent, ki, scale, _ = random_case("ComplEx", 6, 100, 5, seed=11)
    sub = [93, 4, 17, 58, 2, 71, 30]
    got = check(L.COMPLEX, Q, ent, ki, scale, 10, cand=np.unique(sub))
    assert (got[:, 7:] == -1).all() and (got[:, :7] >= 0).all()
    rs = np.random.RandomState(5)
    excl = [rs.choice(100, 30, replace=False) for _ in range(5)]
    got = check(L.COMPLEX, Q, ent, ki, scale, 100, excl=excl)
    assert (got[:, 70:] == -1).all() and (got[:, :70] >= 0).all()
    got = check(L.COMPLEX, Q, ent, ki, scale, 10, cand=np.zeros(0, np.int32))
    assert (got == -1).all()


def test_no_rows():
    d = dev()
    Q, ent, ki, scale, _ = random_case("DistMult", 8, 50, 3, seed=1)
    ids, sc = d.eval_topn(L.DISTMULT, Q[:0], ent, ki, scale, 5)
    assert ids.shape == (0, 5) and sc.shape == (0, 5)


def test_library_refuses_bad_top_n_and_short_workspace():
    d = dev()
    Q, ent, ki, scale, _ = random_case("DistMult", 8, 50, 3, seed=1)
    for bad in (0, NMAX + 1):
        with pytest.raises(L.EmgError, match="top_n"):
            d.eval_topn_ws_bytes(3, 50, bad)
    with pytest.raises(L.EmgError, match="workspace"):
        d.eval_topn(L.DISTMULT, Q, ent, ki, scale, 5, ws=torch.empty(8, dtype=torch.uint8, device="cuda"))


@pytest.mark.parametrize("side", ["o", "s"])
def test_filter_through_topn_device(side):
    """known_csr + topn_device against the dense scores with the known completions removed by a python set"""
    from emgraph_amd.evaluation.ranking import FilterIndex, topn_device
    d = dev()
    name, k, n_ent = "DistMult", 16, 1000
    rs = np.random.RandomState(21)
    E = (rs.randn(n_ent, k) * 0.3).astype(F32)
    R = (rs.randn(4, k) * 0.3).astype(F32)
    ent, rel = table(E), table(R)
    q = np.array([[3, 0], [5, 1], [7, 2], [9, 3]], np.int64)   # (entity, relation); relation 3 is unknown to the filter
    side_mode = L.EVAL_O if side == "o" else L.EVAL_S
    spo = np.zeros((4, 3), np.int32)
    spo[:, 1] = q[:, 1]
    spo[:, 0 if side == "o" else 2] = q[:, 0]
    Q, _ = d.eval_build_queries(L.DISTMULT, ent, rel, k, 1.0, torch.from_numpy(spo).cuda(), side_mode)
    S = d.eval_scores_dense(L.DISTMULT, Q, ent, k, 1.0).cpu().numpy()
    best10 = np.argsort(-S[0], kind="stable")[:10]            # row 0: its 10 best are all known
    hub = rs.choice(n_ent, 500, replace=False)                # row 1: a hub with 500 known completions
    known = [set(best10.tolist()), set(hub.tolist()), {1, 2, 3}, set()]
    trip = [(q[r, 0], q[r, 1], e) if side == "o" else (e, q[r, 1], q[r, 0]) for r in range(3) for e in known[r]]
    trip += [(0, 0, 1), (1, 1, 0)]                            # other keys
    findex = FilterIndex(np.array(trip, np.int64))
    X = q if side == "o" else q[:, ::-1]
    for subset in (None, np.arange(0, n_ent, 2)):             # with a subset: filter entries outside it
        ids_all = np.arange(n_ent) if subset is None else subset
        want_i, want_s = host_topn(S[:, ids_all], ids_all, 10, [sorted(kn) for kn in known])
        got_i, got_s = topn_device(L.DISTMULT, ent, rel, k, 1.0, X, side, 10, filter_triples=findex, entities_subset=subset,
                                   query_chunk=3, ent_chunk=256)
        assert np.array_equal(got_i, want_i) and np.array_equal(got_s.view(np.int32), want_s)
        assert not set(got_i[0].tolist()) & known[0] and not set(got_i[1].tolist()) & known[1]
        assert (got_i >= 0).all()


def test_nan_comes_last_and_only_in_short_rows():
    Q, ent, ki, scale, _ = random_case("DistMult", 8, 100, 4, seed=9)
    ent[17] = float("nan")
    got = check(L.DISTMULT, Q, ent, ki, scale, 100)
    assert (got[:, 99] == 17).all()
    got = check(L.DISTMULT, Q, ent, ki, scale, 99)
    assert (got != 17).all()
    got = check(L.DISTMULT, Q, ent, ki, scale, NMAX)
    assert (got[:, 99] == 17).all() and (got[:, 100:] == -1).all()


@pytest.mark.parametrize("name", ["DistMult", "ComplEx", "TransE_L1"])
def test_literal_oracle_on_dyadic_tables(name):
    """small dyadic values: every score is exact in fp32, so the numpy oracle's scores order the candidates exactly"""
    k, n_ent, rows = 4, 300, 20
    ki, _ = kint_scale(name, k)
    rs = np.random.RandomState(13)
    E = rs.randint(-8, 9, (n_ent, ki)).astype(F32) / 8
    R = rs.randint(-8, 9, (3, ki)).astype(F32) / 8
    Q, ent, ki, scale, spo = queries(name, E, R, k, rows, seed=4)
    x = np.stack([np.repeat(spo[:, 0], n_ent), np.repeat(spo[:, 1], n_ent), np.tile(np.arange(n_ent), rows)], 1).astype(np.int32)
    S = np.asarray(orc.score_triples(name, E, R, x, k=k), F32).reshape(rows, n_ent)
    want_i, _ = host_topn(S, np.arange(n_ent), 10)
    got = check(MODELS[name][0], Q, ent, ki, scale, 10)
    assert np.array_equal(got, want_i)


# ---------------------------------------------------------------- the public function, on a fitted toy model
def toy_graph(n_ent=30, n_rel=3, n=200, seed=0):
    rs = np.random.RandomState(seed)
    X = np.stack([rs.randint(0, n_ent, n), rs.randint(0, n_rel, n), rs.randint(0, n_ent, n)], 1)
    X[:n_ent, 0] = np.arange(n_ent)   # every entity and relation occurs
    X[:n_ent, 2] = np.arange(n_ent)[::-1]
    X[:n_rel, 1] = np.arange(n_rel)
    return np.array([["e%02d" % s, "r%d" % p, "e%02d" % o] for s, p, o in X])


@pytest.mark.parametrize("link", ["linear", "tanh"])
def test_topn_completions_public_api(link):
    from emgraph_amd.evaluation import topn_completions
    from emgraph_amd.models import ComplEx
    from tests.test_hip_kernels import score_tol
    X = toy_graph()
    k = 5
    m = ComplEx(k=k, epochs=1, batches_count=1, seed=3, embedding_model_params={"non_linearity": link})
    m.fit(X)
    for side, cols in (("o", [0, 1]), ("s", [1, 2])):
        q = X[:12, cols]
        labels, scores = topn_completions(q, m, side=side, top_n=10)
        ids, scores_i = topn_completions(np.stack([[m.ent_to_idx[a] if side == "o" else m.rel_to_idx[a] for a in q[:, 0]],
                                                   [m.rel_to_idx[b] if side == "o" else m.ent_to_idx[b] for b in q[:, 1]]], 1),
                                         m, side=side, top_n=10, from_idx=True)
        assert labels.shape == (12, 10) and scores.shape == (12, 10) and scores.dtype == np.float32
        assert np.array_equal(np.vectorize(m.ent_to_idx.get)(labels), ids) and np.array_equal(scores, scores_i)
        trip = np.stack([np.repeat(q[:, 0], 10), np.repeat(q[:, 1], 10), labels.reshape(-1)], 1) if side == "o" else \
            np.stack([labels.reshape(-1), np.repeat(q[:, 0], 10), np.repeat(q[:, 1], 10)], 1)
        pred = m.predict(trip)
        E, R = (np.asarray(t, F32) for t in m.trained_model_params)
        from emgraph_amd.evaluation import to_idx
        tol = score_tol("ComplEx", E, R, to_idx(trip, m.ent_to_idx, m.rel_to_idx), k)   # (the links are 1-Lipschitz)
        assert np.all(np.abs(pred - scores.reshape(-1)) <= tol), np.abs(pred - scores.reshape(-1)).max()
        assert np.all(np.diff(scores, axis=1) <= 0)
    # the filter: the known objects of a query never come back
    labels, _ = topn_completions(X[:12, :2], m, top_n=10, filter_triples=X)
    for r in range(12):
        known = {o for s, p, o in X if s == X[r, 0] and p == X[r, 1]}
        assert not known & set(labels[r].tolist())


def test_position_in_topn_agrees_with_the_ranks():
    from emgraph_amd.models import DistMult
    X = toy_graph(n_ent=100, n_rel=4, n=400, seed=2)
    m = DistMult(k=8, epochs=1, batches_count=1, seed=1)
    m.fit(X)
    from emgraph_amd.evaluation import to_idx
    T = to_idx(X[:50], m.ent_to_idx, m.rel_to_idx)
    ids, _ = m.get_topn_idx(T[:, :2], side="o", top_n=100)
    best = m.get_ranks_idx(T, corrupt_side="o", ranking_strategy="best")
    worst = m.get_ranks_idx(T, corrupt_side="o", ranking_strategy="worst")
    for r in range(len(T)):
        p = int(np.flatnonzero(ids[r] == T[r, 2])[0])
        assert best[r] - 1 <= p <= worst[r] - 1, (r, p, best[r], worst[r])
