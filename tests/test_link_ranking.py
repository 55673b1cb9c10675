"""Ranking THROUGH the score link on the device (embedding_model_params 'non_linearity' + 'rank_through_link'; DESIGN.md 4.2
"Ranking through a link").  The reference applies the link to the positive's and to every corruption's score
(EmbeddingModel.py:1868-1879) and compares int32(phi(score) * 1e5) (:2010-2033).

The exact reference of these tests is the device's OWN link: raw scores from emg_eval_scores_dense pushed through
emg_link_scores (the bits of the training step), the integer formed on the host with float32 arithmetic, counted on the host.
Counters and ranks must be EQUAL (integers: no tolerance).  The float64 interval pin of tests/_link_rank_ref.py (tanh and sigmoid;
softplus is left out there: one float32 ulp of its values is a tenth of a comparison cell) is asserted at the end."""
import functools

import numpy as np
import pytest

from tests import _link_rank_ref as ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import emgraph_oracle as orc  # noqa: E402

F32 = np.float32
LINKS = ("tanh", "sigmoid", "softplus")
MODELS = ("TransE_L1", "TransE_L2", "TransE_P3", "DistMult", "ComplEx", "HolE")
K_MIN, K_MAX = 0x007FFFFF, 0xFF800000        # ordered keys of -inf and +inf (include/emgraph_hip.h)


def _libs():
    from emgraph_amd import _lib as L
    from emgraph_amd import device as D
    D.require_gpu()
    return L, D


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _mid(model):
    L, _ = _libs()
    return L.TRANSE_P if model.startswith("TransE_P") else orc.MODEL_IDS[model]


def _scale(model, k):
    return 3.0 if model.startswith("TransE_P") else (float(F32(2 / k)) if model == "HolE" else 1.0)   # (TransE_P: the order of the norm)


def _kint(model, k):
    return 2 * k if model in ("ComplEx", "HolE") else k


def _tables(model, k, n_ent, n_rel, seed, sigma=None):
    """tables whose raw scores are of order one at any width: where the links are NOT saturated and the integers are dense"""
    rs = np.random.RandomState(seed)
    ki = _kint(model, k)
    if sigma is None:
        sigma = 1.5 / k if model.startswith("TransE") else ((4.0 * k) ** (-1 / 6) if ki != k else float(k) ** (-1 / 6))
    return (rs.randn(n_ent, ki) * sigma).astype(F32), (rs.randn(n_rel, ki) * sigma).astype(F32), ki


def _cmp_int_host(phi):
    """int32(f32(phi) * f32(1e5)) with float32 arithmetic (values far inside the int32 range)"""
    return (phi.astype(F32) * F32(100000.0)).astype(np.int32)


def _linked_ints(model, link, E, R, ki, sc, T, side_mode):
    """(c [n_rows, n_ent], p [n_rows]) on the host from the device's raw dense scores and the device's link bits"""
    L, D = _libs()
    Et, Rt = cu(E), cu(R)
    Q, _ = D.eval_build_queries(_mid(model), Et, Rt, ki, sc, cu(T), side_mode)
    S = D.eval_scores_dense(_mid(model), Q, Et, ki, sc)
    n_rows, n_ent = S.shape
    nq = len(T)
    tgt = {L.EVAL_S: T[:, 0], L.EVAL_O: T[:, 2]}.get(side_mode, np.concatenate([T[:, 2], T[:, 0]]))
    pos = S[torch.arange(n_rows, device="cuda"), cu(tgt.astype(np.int64))].contiguous()
    raw = S.cpu().numpy().copy()
    neg = S.reshape(-1).contiguous()
    D.link_scores(L.LINK_IDS[link], None, 0.0, pos, neg, n_rows, n_ent)      # in place: weight 1 * phi(score)
    assert nq * (2 if side_mode >= L.EVAL_SPO else 1) == n_rows
    return _cmp_int_host(neg.cpu().numpy().reshape(n_rows, n_ent)), _cmp_int_host(pos.cpu().numpy()), raw


def _host_ranks(c, p, T, side, strategy, n_ent, F=None, subset=None):
    """ranks from the host integers through the package's own host assembly (FilterIndex.csr, ranks_from_counts: pinned on the
    reference by tests/test_oracle_golden.py)"""
    L, _ = _libs()
    from emgraph_amd.evaluation.ranking import FilterIndex, ranks_from_counts
    cols = np.arange(n_ent) if subset is None else np.asarray(subset)
    gt = (c[:, cols] > p[:, None]).sum(1)
    eq = (c[:, cols] == p[:, None]).sum(1)
    fgt, feq = np.zeros_like(gt), np.zeros_like(eq)
    if F is not None:
        ptr, idx = FilterIndex(F).csr(T, L.EVAL_SIDE_IDS[side], n_ent, subset)
        for r in range(len(p)):
            ci = c[r, idx[ptr[r]:ptr[r + 1]]]
            fgt[r], feq[r] = (ci > p[r]).sum(), (ci == p[r]).sum()
    return ranks_from_counts(gt, eq, fgt, feq, len(T), side, strategy), gt, eq


@functools.lru_cache(maxsize=None)
def _case(model, k):
    """one table set per (model, width), shared by the links: 700 entities, 70 test triples, a filter, a candidate subset"""
    n_ent, nq = 700, 70
    E, R, ki = _tables(model, k, n_ent, 5, seed=11 * k + len(model))
    rs = np.random.RandomState(k + 1)
    T = np.stack([rs.randint(0, n_ent, nq), rs.randint(0, 5, nq), rs.randint(0, n_ent, nq)], 1).astype(np.int32)
    for j in range(0, nq, 5):                       # exact ties: other entities carry a true entity's row
        E[rs.randint(0, n_ent, 2)] = E[T[j, 2]]
        E[rs.randint(0, n_ent, 1)] = E[T[j, 0]]
    F = np.concatenate([T, np.stack([rs.randint(0, n_ent, 3000), rs.randint(0, 5, 3000), rs.randint(0, n_ent, 3000)], 1)]).astype(np.int32)
    subset = np.unique(rs.randint(0, n_ent, 333)).astype(np.int32)
    return E, R, ki, T, F, subset


# ---- 1. the exact kernels against the device's own link bits ---------------------------------------------------------------------
@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("k", [8, 50])
@pytest.mark.parametrize("model", MODELS)
def test_exact_counts_and_ranks_equal_the_device_link_bits(model, k, link):
    L, D = _libs()
    from emgraph_amd.evaluation import rank_triples_device
    E, R, ki, T, F, subset = _case(model, k)
    n_ent, sc, lk, mid = E.shape[0], _scale(model, k), L.LINK_IDS[link], _mid(model)
    Et, Rt = cu(E), cu(R)
    # counters of the C-ABI calls, rows of both sides
    c, p, _ = _linked_ints(model, link, E, R, ki, sc, T, L.EVAL_S_O)
    Q, pos_int = D.eval_build_queries(mid, Et, Rt, ki, sc, cu(T), L.EVAL_S_O, link=lk)
    np.testing.assert_array_equal(pos_int.cpu().numpy(), p)
    n_rows = Q.shape[0]
    cnt = torch.zeros((4, n_rows), dtype=torch.int32, device="cuda")
    D.eval_count(mid, Q, pos_int, Et, ki, sc, cnt[0], cnt[1], link=lk)
    np.testing.assert_array_equal(cnt[0].cpu().numpy(), (c > p[:, None]).sum(1))
    np.testing.assert_array_equal(cnt[1].cpu().numpy(), (c == p[:, None]).sum(1))
    assert (c == p[:, None]).sum(1).min() >= 1              # the positive ties with itself
    cnt.zero_()
    D.eval_count(mid, Q, pos_int, Et, ki, sc, cnt[0], cnt[1], cand=cu(subset), link=lk)
    np.testing.assert_array_equal(cnt[0].cpu().numpy(), (c[:, subset] > p[:, None]).sum(1))
    np.testing.assert_array_equal(cnt[1].cpu().numpy(), (c[:, subset] == p[:, None]).sum(1))
    from emgraph_amd.evaluation.ranking import FilterIndex
    ptr, idx = FilterIndex(F).csr(T, L.EVAL_S_O, n_ent)
    D.eval_filter_count(mid, Q, pos_int, Et, 0, ki, sc, cu(ptr), cu(idx), cnt[2], cnt[3], link=lk)
    fgt = np.array([(c[r, idx[ptr[r]:ptr[r + 1]]] > p[r]).sum() for r in range(n_rows)])
    feq = np.array([(c[r, idx[ptr[r]:ptr[r + 1]]] == p[r]).sum() for r in range(n_rows)])
    np.testing.assert_array_equal(cnt[2].cpu().numpy(), fgt)
    np.testing.assert_array_equal(cnt[3].cpu().numpy(), feq)
    # ranks of the whole path: sides, strategies, filter, candidate subset
    for side in ("s,o", "s+o", "o"):
        cs, ps, _ = (c, p, None) if side != "o" else _linked_ints(model, link, E, R, ki, sc, T, L.EVAL_O)
        for strategy in ("worst", "best", "middle"):
            for filt in (None, F):
                for sub in (None, subset):
                    want, _, _ = _host_ranks(cs, ps, T, side, strategy, n_ent, filt, sub)
                    got = rank_triples_device(mid, Et, Rt, ki, sc, T, side, strategy, filter_triples=filt, entities_subset=sub, link=lk)
                    np.testing.assert_array_equal(got, want, err_msg=str((side, strategy, filt is not None, sub is not None)))


def test_link_ids_outside_the_table_are_refused():
    L, D = _libs()
    E, R, ki, T, F, subset = _case("DistMult", 8)
    Et, Rt = cu(E), cu(R)
    Q, pos_int = D.eval_build_queries(L.DISTMULT, Et, Rt, ki, 1.0, cu(T), L.EVAL_O)
    cnt = torch.zeros((2, Q.shape[0]), dtype=torch.int32, device="cuda")
    for bad in (-1, 4, 17):
        with pytest.raises(L.EmgError):
            D.eval_build_queries(L.DISTMULT, Et, Rt, ki, 1.0, cu(T), L.EVAL_O, link=bad)
        with pytest.raises(L.EmgError):
            D.eval_count(L.DISTMULT, Q, pos_int, Et, ki, 1.0, cnt[0], cnt[1], link=bad)
        with pytest.raises(L.EmgError):
            D.eval_link_thresholds(bad, pos_int, None, 1.0)
    assert int(cnt.abs().sum()) == 0


# ---- 2. saturation: the link turns whole stretches of the score axis into ties -----------------------------------------------------
def _saturated_tables(model, k, n_ent, link, seed):
    """tables whose raw scores ALL lie where the link's integer no longer moves: above 18 (tanh rounds to 1.0f above ~9.1, the
    sigmoid above ~17.4: integer 100000) or below -25 (custom_softplus * 1e5 < 1 below -20.73: integer 0).  All entries positive,
    so every term of a contraction has one sign; the relation rows are negated for the negative stretch."""
    rs = np.random.RandomState(seed)
    ki = _kint(model, k)
    per_coord = {"DistMult": 1.0, "ComplEx": 2.0, "HolE": 2.0}[model] * (2.0 / k if model == "HolE" else 1.0)   # score ~ per_coord k a^3
    a = (30.0 / (per_coord * k)) ** (1 / 3)
    E = (a * (1.0 + 0.15 * rs.rand(n_ent, ki))).astype(F32)
    R = (a * (1.0 + 0.15 * rs.rand(3, ki))).astype(F32)
    return E, (-R if link == "softplus" else R), ki


@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("model,k", [("DistMult", 8), ("DistMult", 50), ("ComplEx", 50)])
def test_saturation_makes_mass_ties_and_they_are_counted(model, k, link):
    L, D = _libs()
    from emgraph_amd.evaluation import rank_triples_device
    n_ent, nq = 700, 70
    E, R, ki = _saturated_tables(model, k, n_ent, link, seed=k)
    rs = np.random.RandomState(3)
    T = np.stack([rs.randint(0, n_ent, nq), rs.randint(0, 3, nq), rs.randint(0, n_ent, nq)], 1).astype(np.int32)
    sc, lk, mid = _scale(model, k), L.LINK_IDS[link], _mid(model)
    c, p, raw = _linked_ints(model, link, E, R, ki, sc, T, L.EVAL_S_O)
    print(model, k, link, "raw scores in [%.2f, %.2f]" % (raw.min(), raw.max()))
    assert (raw.max() < -25.0) if link == "softplus" else (raw.min() > 18.0)          # the construction's promise
    Et, Rt = cu(E), cu(R)
    worst = rank_triples_device(mid, Et, Rt, ki, sc, T, "s,o", "worst", link=lk)
    best = rank_triples_device(mid, Et, Rt, ki, sc, T, "s,o", "best", link=lk)
    want_w, _, eq = _host_ranks(c, p, T, "s,o", "worst", n_ent)
    want_b, _, _ = _host_ranks(c, p, T, "s,o", "best", n_ent)
    np.testing.assert_array_equal(worst, want_w)
    np.testing.assert_array_equal(best, want_b)
    # every candidate ties with the positive: worst - best = the host's count of ties = all 700 entities, on both sides
    np.testing.assert_array_equal((worst - best)[:, 1], eq[:nq])
    np.testing.assert_array_equal((worst - best)[:, 0], eq[nq:])
    assert (eq == n_ent).all() and (best == 1).all()
    # the same tables under the linear link: the raw scores differ, hardly any ties
    lin_w = rank_triples_device(mid, Et, Rt, ki, sc, T, "s,o", "worst")
    lin_b = rank_triples_device(mid, Et, Rt, ki, sc, T, "s,o", "best")
    assert (lin_w - lin_b).max() <= 3


# ---- 3. precision 2 == precision 0 under a link --------------------------------------------------------------------------------------
@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("model,k,n_ent,nq,scale", [("ComplEx", 200, 30000, 300, 0.1), ("DistMult", 128, 5000, 140, 0.05),
                                                     ("HolE", 30, 20000, 170, 0.3), ("ComplEx", 330, 4000, 70, 0.1),
                                                     ("DistMult", 801, 3000, 130, 0.1)])
def test_prefilter_ranks_equal_exact_ranks_under_a_link(model, k, n_ent, nq, scale, link):
    """the layout of tests/test_hip_kernels.py::test_prefilter_ranks_equal_exact_ranks (planted duplicates of the true rows, every
    side, strategy and filter setting) with the link: bit for bit; k_int = 660 is the wide form, 801 is outside the kernel and
    must fall back"""
    L, D = _libs()
    from emgraph_amd.evaluation import rank_triples_device
    rs = np.random.RandomState(k + n_ent)
    ki = _kint(model, k)
    E, R = (rs.randn(n_ent, ki) * scale).astype(F32), (rs.randn(5, ki) * scale).astype(F32)
    rs = np.random.RandomState(n_ent)
    T = np.stack([rs.randint(0, n_ent, nq), rs.randint(0, 5, nq), rs.randint(0, n_ent, nq)], 1).astype(np.int32)
    for j in range(0, nq, 4):
        E[rs.randint(0, n_ent, 2)] = E[T[j, 2]]
        E[rs.randint(0, n_ent, 1)] = E[T[j, 0]]
    F = np.concatenate([T, np.stack([rs.randint(0, n_ent, 5000), rs.randint(0, 5, 5000), rs.randint(0, n_ent, 5000)], 1)]).astype(np.int32)
    sc, lk, mid = _scale(model, k), L.LINK_IDS[link], _mid(model)
    Et, Rt = cu(E), cu(R)
    used = 0
    for side in ("s,o", "s+o", "o"):
        for strategy in ("worst", "best", "middle"):
            for filt in (None, F):
                st = {}
                exact = rank_triples_device(mid, Et, Rt, ki, sc, T, side, strategy, filter_triples=filt, link=lk)
                fast = rank_triples_device(mid, Et, Rt, ki, sc, T, side, strategy, filter_triples=filt, precision=2, stats=st, link=lk)
                np.testing.assert_array_equal(fast, exact, err_msg=str((side, strategy, filt is not None)))
                used += st.get("pairs", 0) + st.get("fallback", 0)
    if D.link_order_w(lk) > 0 and ki <= 800 and 2 * nq > 128:
        assert used > 0        # the prefilter ran and handed candidates (at least the ties) to the exact re-scoring


@pytest.mark.parametrize("model", ["TransE_L1", "TransE_L2"])
def test_transe_under_a_link_takes_the_exact_kernel(model):
    L, D = _libs()
    from emgraph_amd.evaluation import rank_triples_device
    E, R, ki = _tables(model, 64, 3000, 4, seed=5)
    rs = np.random.RandomState(1)
    T = np.stack([rs.randint(0, 3000, 150), rs.randint(0, 4, 150), rs.randint(0, 3000, 150)], 1).astype(np.int32)
    Et, Rt = cu(E), cu(R)
    exact = rank_triples_device(_mid(model), Et, Rt, ki, 1.0, T, link=L.LINK_SIGMOID)
    for prec in (2, "auto"):
        st = {}
        np.testing.assert_array_equal(rank_triples_device(_mid(model), Et, Rt, ki, 1.0, T, precision=prec, stats=st, link=L.LINK_SIGMOID), exact)
        assert st.get("link_exact_only") is True
        assert "pairs" not in st
    with pytest.raises(NotImplementedError):
        rank_triples_device(L.DISTMULT, Et, Rt, ki, 1.0, T, precision=1, link=L.LINK_SIGMOID)


# ---- 4. proven ties under saturation ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("link", ["tanh", "softplus"])
@pytest.mark.parametrize("model", ["ComplEx", "DistMult"])
def test_saturated_tables_are_decided_by_proven_ties(model, link, monkeypatch):
    L, D = _libs()
    from emgraph_amd.evaluation import rank_triples_device
    if D.link_order_w(L.LINK_IDS[link]) == 0:
        pytest.skip("no order slack for this link: exact kernel only")   # (not the case with the committed constants)
    n_ent, nq, k = 30000, 260, 200
    E, R, ki = _saturated_tables(model, k, n_ent, link, seed=7)
    rs = np.random.RandomState(9)
    T = np.stack([rs.randint(0, n_ent, nq), rs.randint(0, 3, nq), rs.randint(0, n_ent, nq)], 1).astype(np.int32)
    sc, lk, mid = _scale(model, k), L.LINK_IDS[link], _mid(model)
    Et, Rt = cu(E), cu(R)
    exact_w = rank_triples_device(mid, Et, Rt, ki, sc, T, "s,o", "worst", link=lk)
    exact_b = rank_triples_device(mid, Et, Rt, ki, sc, T, "s,o", "best", link=lk)
    assert ((exact_w - exact_b) == n_ent).all()      # the pure case: every candidate ties with the positive
    for strategy, exact in (("worst", exact_w), ("best", exact_b)):
        st = {}
        fast = rank_triples_device(mid, Et, Rt, ki, sc, T, "s,o", strategy, precision=2, stats=st, link=lk)
        np.testing.assert_array_equal(fast, exact)
        print(model, link, strategy, st)
        assert st["prove_ties"] is True
        assert st.get("fallback", 0) == 0
    monkeypatch.setenv("EMG_PREFILTER_TIES", "0")
    st = {}
    fast = rank_triples_device(mid, Et, Rt, ki, sc, T, "s,o", "worst", precision=2, stats=st, link=lk)
    np.testing.assert_array_equal(fast, exact_w)
    assert st["prove_ties"] is False and st.get("fallback", 0) > 0


# ---- 5. the threshold kernel ---------------------------------------------------------------------------------------------------------------
def _key_to_float(k):
    k = np.asarray(k, np.uint32)
    bits = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k)
    return bits.astype(np.uint32).view(F32)


def _float_to_key(x):
    u = np.asarray(x, F32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _c_of(link, x):
    """the device's comparison integer of the raw scores x (emg_link_scores bits, float32 host multiply)"""
    L, D = _libs()
    x = np.ascontiguousarray(x, F32).reshape(-1)
    pos, neg = cu(x[:1].copy()), cu(x.copy())
    D.link_scores(L.LINK_IDS[link], None, 0.0, pos, neg, 1, len(x))
    with np.errstate(invalid="ignore", over="ignore"):
        v = neg.cpu().numpy().astype(F32) * F32(100000.0)
    return np.where(v >= 2147483648.0, np.int64(2147483647), np.where(v <= -2147483648.0, np.int64(-2147483648), np.trunc(v))).astype(np.int64)


@pytest.mark.parametrize("link", LINKS)
def test_link_thresholds_bracket_the_cell_edges(link):
    """512 rows: positives at cell edges (the integers of scores spread over the link's live range), at 0, at the saturated ends,
    beyond them (nothing greater / nothing smaller) and at the integers of +-inf.  For every finite score-domain threshold the
    device's c is scanned over the 4096 floats around it: above G_out everything is greater, below E_out smaller, inside
    [E_in, G_in] a tie; the undecided zones are at most 2 W + 2 floats wide; an infinite threshold is checked at the axis' end."""
    L, D = _libs()
    lk = L.LINK_IDS[link]
    W = D.link_order_w(lk)
    if W == 0:
        pytest.skip("no order slack for this link: exact kernel only")
    rs = np.random.RandomState(4)
    xs = np.concatenate([rs.uniform(-30, 30, 400), rs.uniform(-1e-3, 1e-3, 40), [0.0, -0.0, 6.1, 9.2, 17.5, -20.7, -25.0, 79.0]]).astype(F32)
    c_inf = _c_of(link, np.array([-np.inf, np.inf], F32))
    special = [0, 1, -1, 99998, 99999, 100000, 100001, -99999, -100000, -100001, 2147483647, -2147483647, int(c_inf[0]), int(c_inf[1])]
    p = np.concatenate([_c_of(link, xs), special]).astype(np.int64)
    p = np.concatenate([p, p[: 512 - len(p)] + rs.randint(-1, 2, 512 - len(p))]).clip(-2147483647, 2147483647).astype(np.int32)
    assert len(p) == 512
    _, _, ts = D.eval_link_thresholds(lk, cu(p), None, 1.0)
    g_out, e_out, g_in, e_in = ts.cpu().numpy().reshape(4, 512)
    assert not np.isnan(ts.cpu().numpy()).any()
    kg_out, ke_out, kg_in, ke_in = (_float_to_key(t).astype(np.int64) for t in (g_out, e_out, g_in, e_in))
    fin = lambda t: np.isfinite(t)   # noqa: E731
    # widths of the undecided zones (floats strictly between the inner and the outer threshold)
    both = fin(g_out) & fin(g_in)
    assert both.sum() > 300 and ((kg_out - kg_in - 1)[both] <= 2 * W + 2).all() and ((kg_out - kg_in)[both] >= 1).all()
    both = fin(e_out) & fin(e_in)
    assert both.sum() > 300 and ((ke_in - ke_out - 1)[both] <= 2 * W + 2).all() and ((ke_in - ke_out)[both] >= 1).all()
    # the four implications on the floats around every finite threshold
    off = np.arange(-2048, 2048, dtype=np.int64)
    for thr_keys, finite in ((kg_out, fin(g_out)), (ke_out, fin(e_out)), (kg_in, fin(g_in)), (ke_in, fin(e_in))):
        rows = np.nonzero(finite)[0]
        keys = np.clip(thr_keys[rows, None] + off[None, :], K_MIN, K_MAX)
        c = _c_of(link, _key_to_float(keys.astype(np.uint32))).reshape(keys.shape)
        pr = p[rows, None].astype(np.int64)
        assert (c[keys >= kg_out[rows, None]] > np.broadcast_to(pr, c.shape)[keys >= kg_out[rows, None]]).all()
        assert (c[keys <= ke_out[rows, None]] < np.broadcast_to(pr, c.shape)[keys <= ke_out[rows, None]]).all()
        tie = (keys >= ke_in[rows, None]) & (keys <= kg_in[rows, None])
        assert (c[tie] == np.broadcast_to(pr, c.shape)[tie]).all()
    # no edge on a side: the end of the axis says why
    p64 = p.astype(np.int64)
    assert (c_inf[1] <= p64)[(g_out == np.inf) & (g_in == np.inf)].all()   # nothing is greater: not even +inf
    assert (c_inf[0] > p64)[g_out == -np.inf].all()                      # everything is greater: even -inf
    assert (c_inf[0] >= p64)[(e_out == -np.inf) & (e_in == -np.inf)].all()
    assert (c_inf[1] < p64)[e_out == np.inf].all()
    # accumulator domain at scale 1 and band 0: the thresholds move outwards (inner ones inwards) by the relative slack only
    band = torch.zeros(512, dtype=torch.float32, device="cuda")
    thr, thr4, _ = D.eval_link_thresholds(lk, cu(p), band, 1.0)
    t4 = thr4.cpu().numpy().reshape(4, 512)
    np.testing.assert_array_equal(thr.cpu().numpy(), thr4.cpu().numpy()[:1024])
    assert (t4[0] >= g_out).all() and (t4[1] <= np.nextafter(e_out, F32(np.inf))).all()
    assert (t4[2] <= np.nextafter(g_in, F32(np.inf))).all() and (t4[3] >= e_in).all()
    assert (t4[3] >= t4[1]).all() and (t4[2] <= t4[0]).all()


# ---- 6. the order check ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("link", LINKS)
def test_committed_order_slack_holds_for_every_float(link):
    """the exhaustive sweep (all non-NaN floats, -inf and +inf, both zeros) at the committed W: a proof for this libm, repeated
    here so that another libm cannot break the threshold bisection silently"""
    L, D = _libs()
    lk = L.LINK_IDS[link]
    W = D.link_order_w(lk)
    if W == 0:
        pytest.skip("no order slack for this link: exact kernel only")
    assert W in (1, 2, 4, 8, 16, 32)
    assert int(D.eval_link_order_violations(lk, W).cpu()[0]) == 0


def test_order_check_sees_a_planted_violation():
    """link | 0x100 negates c: every step of tanh's integer is then a violation, at any W; an empty or NaN range is refused"""
    L, D = _libs()
    n1 = int(D.eval_link_order_violations(L.LINK_TANH | 0x100, 1).cpu()[0])
    assert n1 >= 100000                      # -(c >> 1) runs from 50000 down to -50000: at least one violation per step at W = 1
    lo, hi = (int(np.array([v], F32).view(np.uint32)[0]) for v in (0.5, 0.5001))
    n = int(D.eval_link_order_violations(L.LINK_TANH | 0x100, 4, lo, hi).cpu()[0])
    assert 0 < n < n1 * 4
    assert int(D.eval_link_order_violations(L.LINK_LINEAR, 1, lo, hi).cpu()[0]) == 0
    for bad in ((hi, lo), (0x7FC00000, 0x7FC00000)):
        with pytest.raises(L.EmgError):
            D.eval_link_order_violations(L.LINK_TANH, 1, *bad)
    with pytest.raises(L.EmgError):
        D.eval_link_order_violations(L.LINK_TANH, 33)


# ---- 7. the public API -------------------------------------------------------------------------------------------------------------------
N_ENT, N_REL, N_TRIPLES = 300, 5, 2047


def _graph():
    rs = np.random.RandomState(100)
    X = np.stack([rs.randint(0, N_ENT, N_TRIPLES), rs.randint(0, N_REL, N_TRIPLES), rs.randint(0, N_ENT, N_TRIPLES)], 1)
    X[:N_ENT, 0] = np.arange(N_ENT)                      # every entity and relation occurs: labels == ids after mapping
    X[:N_REL, 1] = np.arange(N_REL)
    return X.astype(np.int64)


def _model(name, emp, epochs=2, lr=0.05, k=16):
    from emgraph_amd import models
    E0, R0, _ = _tables(name, k, N_ENT, N_REL, seed=40 + k)
    params = {"corrupt_side": "s,o"}
    params.update(emp)
    return getattr(models, name)(k=k, eta=2, epochs=epochs, batches_count=4, seed=5, loss="nll", optimizer="sgd",
                                 optimizer_params={"lr": lr}, embedding_model_params=params, initializer="constant",
                                 initializer_params={"entity": E0, "relation": R0})


@pytest.mark.parametrize("name", ["DistMult", "ComplEx"])
def test_public_api_ranks_through_the_link(name):
    L, D = _libs()
    from emgraph_amd.evaluation import evaluate_performance, rank_triples_device
    X = _graph()
    m = _model(name, {"non_linearity": "tanh", "rank_through_link": True, "eval_precision": 0})
    m.fit(X)
    E, R = (np.asarray(a, F32) for a in m.trained_model_params[:2])
    ki = E.shape[1]
    Xi = np.stack([[m.ent_to_idx[s] for s in X[:120, 0]], [m.rel_to_idx[r] for r in X[:120, 1]], [m.ent_to_idx[o] for o in X[:120, 2]]], 1)
    Fi = np.stack([[m.ent_to_idx[s] for s in X[:, 0]], [m.rel_to_idx[r] for r in X[:, 1]], [m.ent_to_idx[o] for o in X[:, 2]]], 1)
    want = rank_triples_device(_mid(name), cu(E), cu(R), ki, 1.0, Xi, "s,o", "worst", filter_triples=Fi, link=L.LINK_TANH)
    linear = rank_triples_device(_mid(name), cu(E), cu(R), ki, 1.0, Xi, "s,o", "worst", filter_triples=Fi)
    for prec in (0, 2, "auto"):
        m.embedding_model_params["eval_precision"] = prec
        got = evaluate_performance(X[:120], m, filter_triples=X)
        np.testing.assert_array_equal(np.asarray(got).reshape(want.shape), want, err_msg=str(prec))
    assert want.shape == linear.shape     # (the linear ranks of the same tables: computed by the same call without the link)
    m.embedding_model_params["eval_precision"] = 1
    with pytest.raises(NotImplementedError):
        evaluate_performance(X[:120], m, filter_triples=X)
    # the same model without the key: refused as ever, and the message names the key
    m2 = _model(name, {"non_linearity": "tanh"})
    m2.fit(X)
    with pytest.raises(NotImplementedError, match="non_linearity") as ei:
        evaluate_performance(X[:8], m2, filter_triples=X)
    assert "rank_through_link" in str(ei.value)
    with pytest.raises(NotImplementedError, match="non_linearity"):
        m2.fit(X, early_stopping=True, early_stopping_params={"x_valid": X[:8]})
    for bad in (1, "yes"):
        with pytest.raises(ValueError, match="rank_through_link"):
            evaluate_performance(X[:8], _fitted_like(m, bad), filter_triples=X)


def _fitted_like(m, key_value):
    m.embedding_model_params["rank_through_link"] = key_value
    return m


@pytest.mark.parametrize("name", ["DistMult", "ComplEx"])
def test_early_stopping_ranks_through_the_link(name):
    """a learning rate too small to move a rank: the criterion never improves, so the fit stops after stop_interval checks"""
    X = _graph()
    m = _model(name, {"non_linearity": "tanh", "rank_through_link": True}, epochs=30, lr=1e-12)
    m.fit(X, early_stopping=True, early_stopping_params={"x_valid": X[:64], "criteria": "mrr", "burn_in": 0, "check_interval": 1,
                                                         "stop_interval": 2, "x_filter": X})
    assert m.early_stopping_epoch is not None and m.early_stopping_epoch <= 4
    assert m.is_fitted


# ---- the float64 interval pin (tests/_link_rank_ref.py) ---------------------------------------------------------------------------------
@pytest.mark.parametrize("link", ref.LINKS)
@pytest.mark.parametrize("name", ["TransE", "DistMult", "ComplEx", "HolE"])
def test_device_ranks_lie_inside_the_float64_intervals(golden, name, link):
    """tanh and sigmoid on the golden rank tables, raw and filtered 'worst' ranks (softplus: see the helper's docstring)"""
    L, D = _libs()
    from emgraph_amd.evaluation import rank_triples_device
    g = golden("ranks")
    E, R, F, T = g["rk_%s_E" % name], g["rk_%s_R" % name], g["flt_filter"], g["flt_test"]
    om = "TransE_L1" if name == "TransE" else name
    sc = _scale(om, 4)
    lists = dict(obj_ptr=g["flt_obj_ptr"], obj_idx=g["flt_obj_idx"], sub_ptr=g["flt_sub_ptr"], sub_idx=g["flt_sub_idx"])
    for filt, kw in ((None, {}), (F, lists)):
        lo, hi = ref.rank_intervals(name, link, E, R, T, **kw)
        got = rank_triples_device(_mid(om), cu(E), cu(R), E.shape[1], sc, T, "s,o", "worst", filter_triples=filt, link=L.LINK_IDS[link])
        assert ((lo <= got) & (got <= hi)).all(), (got, lo, hi)
