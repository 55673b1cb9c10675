"""SimplE (EMG_SIMPLE) on the device against the host references of tests/_simple_ref.py: scores and gradients of the generic kernels
against float64 within derived bounds, the query rows and every 1-vs-all path TO THE BIT against the committed C chain, the
exact-fast mode against the exact kernel, the relation side against the object side, one optimizer step, the one-call step, the
refusals, and the public API.

Shapes (tests/_simple_ref.py): 130 positives / query rows over 300 entities and 6 relations — past the 64- and 128-row tile edges and
two 128-candidate tiles; k = 1, 5 (k_int = 10: no multiple of 4), 37 (the half boundary at a column that is no multiple of 4), 64
(a lane per column of a half), 200 (several columns per lane); eta up to 82 (more negatives than a wave has lanes).  Table padding
is NaN: a read past k_int, or a half swapped at the wrong column, shows in every comparison."""
import functools

import numpy as np
import pytest

from tests import _relrank_ref as relref
from tests import _simple_ref as ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32 = np.float32
SC = ref.SCALE
N_ENT, N_REL, B = ref.N_ENT, ref.N_REL, ref.N_POS


def _libs():
    from emgraph_amd import _lib as L
    from emgraph_amd import device as D
    D.require_gpu()
    return L, D


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def table(a, ld=None):
    """a device table holding ``a``, its padding NaN: row stride padded to 16 bytes AND at least one float of padding, or ``ld`` floats
    (an odd one: rows of no alignment)"""
    n, k = a.shape
    buf = torch.full((n, ld or ((k + 4) // 4) * 4), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :k] = cu(a)
    return buf[:, :k]


@functools.lru_cache(maxsize=None)
def _case(k, eta):
    return ref.training_case(k, eta)


# ---- 1. the generic kernels against float64 --------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,eta,aligned", [(k, eta, (k + eta) % 2 == 0) for k in (1, 5, 37, 64, 200) for eta in (1, 2, 5)]
                         + [(5, 2, False), (64, 1, True), (65, 82, True), (65, 82, False)])
def test_scores_and_gradients_vs_float64(k, eta, aligned):
    """scores within ref.score_bound, gradient rows (accumulated into tables in float64 by the test) within ref.grad_bound — both
    derived there, neither tuned; the forward's positive scores are emg_score_triples' bits"""
    L, D = _libs()
    E, R, X, codes, xneg, _, _ = _case(k, eta)
    assert X[0, 0] == X[0, 2] and xneg[1, 0] == xneg[1, 2] and xneg[2, 0] == xneg[2, 2]
    ki = 2 * k
    ld = None if aligned else ki + 3                             # an odd stride: rows of no alignment
    Et, Rt, Xt, ct = table(E, ld), table(R, ld), cu(X), cu(codes)
    assert (Et.stride(0) % 4 == 0) == aligned and Et.stride(0) > ki
    sp, sn = D.train_forward(L.SIMPLE, Et, Rt, ki, SC, Xt, eta, ct)
    sp, sn = sp.cpu().numpy(), sn.cpu().numpy()
    worst = 0.0
    for got, T in ((sp, X), (sn, xneg)):
        err, bound = np.abs(got.astype(np.float64) - ref.score_f64(E, R, T)), ref.score_bound(E, R, T)
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound)
    np.testing.assert_array_equal(D.score_triples(L.SIMPLE, Et, Rt, ki, SC, Xt).cpu().numpy(), sp)
    np.testing.assert_array_equal(D.score_triples(L.SIMPLE, Et, Rt, ki, SC, cu(xneg)).cpu().numpy(), sn)

    rs = np.random.RandomState(k + eta)
    gpos = rs.randn(B).astype(F32)
    gneg = rs.randn(B * eta).astype(F32)
    ldc = ((ki + 3) // 4) * 4 if aligned else ki + 1
    ce = torch.full(((2 + eta) * B, ldc), 7.0, dtype=torch.float32, device="cuda")    # (every slot is written, not accumulated into)
    cr = torch.full((B, ldc), 7.0, dtype=torch.float32, device="cuda")
    de = torch.empty((2 + eta) * B, dtype=torch.int32, device="cuda")
    dr = torch.empty(B, dtype=torch.int32, device="cuda")
    D.train_backward(L.SIMPLE, Et, Rt, ki, SC, Xt, eta, ct, cu(gpos), cu(gneg), ce[:, :ki], cr[:, :ki], de, dr)
    ce, cr = ce.cpu().numpy(), cr.cpu().numpy()
    assert np.all(ce[:, ki:] == 7.0) and np.all(cr[:, ki:] == 7.0)                    # nothing past k_int is written
    ce, cr = ce[:, :ki], cr[:, :ki]
    assert np.all(np.isfinite(ce)) and np.all(np.isfinite(cr))
    dE = np.zeros((N_ENT, ki))
    dR = np.zeros((N_REL, ki))
    np.add.at(dE, de.cpu().numpy(), ce.astype(np.float64))
    np.add.at(dR, dr.cpu().numpy(), cr.astype(np.float64))
    T, g = np.concatenate([X, xneg]), np.concatenate([gpos, gneg])
    eE, eR = ref.grads_f64(E, R, T, g)
    bE, bR = ref.grad_bound(E, R, T, g, eta)
    worst_g = max(float((np.abs(dE - eE)[bE > 0] / bE[bE > 0]).max()), float((np.abs(dR - eR)[bR > 0] / bR[bR > 0]).max()))
    print("k=%d eta=%d aligned=%s: worst score error %.3f of its bound, worst gradient error %.3f of its bound" % (k, eta, aligned, worst, worst_g))
    assert np.all(np.abs(dE - eE) <= bE) and np.all(np.abs(dR - eR) <= bR)


# ---- 2. query rows ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 5, 37, 64, 200])
@pytest.mark.parametrize("aligned", [True, False])
def test_query_rows_equal_the_single_rounding_products(k, aligned):
    L, D = _libs()
    E, R, X, _, _, _, _ = _case(k, 2)
    ki = 2 * k
    Q, _ = D.eval_build_queries(L.SIMPLE, table(E, None if aligned else ki + 1), table(R, None if aligned else ki + 3), ki, SC, cu(X),
                                L.EVAL_S_O, ldq=None if aligned else ki + 1)
    Q = Q.cpu().numpy()[:, :ki]
    np.testing.assert_array_equal(Q[:B], ref.queries_f32(E, R, X, True))
    np.testing.assert_array_equal(Q[B:], ref.queries_f32(E, R, X, False))


# ---- 3. dense scores, counts and the alias ---------------------------------------------------------------------------------------
def _chain_case(k, aligned=True):
    """(Q device, pos_int device, Et, Rt, S host chain from the device's own query rows, tgt, E, R, X)"""
    L, D = _libs()
    E, R, X, _, _, _, _ = _case(k, 2)
    ki = 2 * k
    Et, Rt = table(E, None if aligned else ki + 1), table(R)
    Q, pos_int = D.eval_build_queries(L.SIMPLE, Et, Rt, ki, SC, cu(X), L.EVAL_S_O, ldq=None if aligned else ki + 3)
    S = ref.chain_f32(Q.cpu().numpy()[:, :ki], E)
    tgt = np.concatenate([X[:, 2], X[:, 0]])
    return Q, pos_int, Et, Rt, S, tgt, E, R, X


@pytest.mark.parametrize("k", [5, 37, 64, 200])
@pytest.mark.parametrize("aligned", [True, False])
def test_dense_scores_and_counts_equal_the_c_chain(k, aligned):
    L, D = _libs()
    ki = 2 * k
    Q, pos_int, Et, Rt, S, tgt, E, R, X = _chain_case(k, aligned)
    assert (Et.stride(0) % 4 == 0) == aligned and (Q.stride(0) % 4 == 0) == aligned
    got = D.eval_scores_dense(L.SIMPLE, Q, Et, ki, SC)
    np.testing.assert_array_equal(got.cpu().numpy().view(np.int32), S.view(np.int32))
    assert torch.equal(got, D.eval_scores_dense(L.HOLE, Q, Et, ki, SC))              # the alias: HolE's chain on the same operands
    c, p = ref.cmp_int(S), ref.cmp_int(S[np.arange(2 * B), tgt])
    np.testing.assert_array_equal(pos_int.cpu().numpy(), p)
    cnt = torch.zeros((4, 2 * B), dtype=torch.int32, device="cuda")
    D.eval_count(L.SIMPLE, Q, pos_int, Et, ki, SC, cnt[0], cnt[1])
    np.testing.assert_array_equal(cnt[0].cpu().numpy(), (c > p[:, None]).sum(1))
    np.testing.assert_array_equal(cnt[1].cpu().numpy(), (c == p[:, None]).sum(1))
    from emgraph_amd.evaluation.ranking import FilterIndex
    rs = np.random.RandomState(k + 1)
    F = np.concatenate([X, np.stack([rs.randint(0, N_ENT, 900), rs.randint(0, N_REL, 900), rs.randint(0, N_ENT, 900)], 1)]).astype(np.int32)
    ptr, idx = FilterIndex(F).csr(X, L.EVAL_S_O, N_ENT)
    D.eval_filter_count(L.SIMPLE, Q, pos_int, Et, 0, ki, SC, cu(ptr), cu(idx), cnt[2], cnt[3])
    np.testing.assert_array_equal(cnt[2].cpu().numpy(), [(c[r, idx[ptr[r]:ptr[r + 1]]] > p[r]).sum() for r in range(2 * B)])
    np.testing.assert_array_equal(cnt[3].cpu().numpy(), [(c[r, idx[ptr[r]:ptr[r + 1]]] == p[r]).sum() for r in range(2 * B)])


def test_grouped_counts():
    L, D = _libs()
    k = 37
    Q, pos_int, Et, _, S, tgt, *_ = _chain_case(k)
    c, p = ref.cmp_int(S), pos_int.cpu().numpy()
    rs = np.random.RandomState(2)
    pools = [np.zeros(0, np.int32)] + [np.unique(rs.randint(0, N_ENT, n)).astype(np.int32) for n in (1, 40, 290)]
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in pools])]).astype(np.int64)
    idx = np.concatenate(pools).astype(np.int32)
    rg = rs.randint(-1, len(pools), 2 * B).astype(np.int32)
    cnt = torch.zeros((2, 2 * B), dtype=torch.int32, device="cuda")
    D.eval_count_grouped(L.SIMPLE, Q, pos_int, cu(rg), Et, 2 * k, SC, cu(ptr), cu(idx), cnt[0], cnt[1])
    want = np.array([[(c[r, pools[g]] > p[r]).sum() if g >= 0 else 0, (c[r, pools[g]] == p[r]).sum() if g >= 0 else 0] for r, g in enumerate(rg)])
    np.testing.assert_array_equal(cnt.cpu().numpy().T, want)
    assert want[:, 0].max() > 0


def test_list_counts():
    L, D = _libs()
    k, K = 37, 50
    Q, pos_int, Et, _, S, tgt, *_ = _chain_case(k)
    c, p = ref.cmp_int(S), pos_int.cpu().numpy()
    cand = np.random.RandomState(3).randint(0, N_ENT, (2 * B, K)).astype(np.int32)
    cand[:, 0] = tgt
    cnt = torch.zeros((2, 2 * B), dtype=torch.int32, device="cuda")
    D.eval_count_lists(L.SIMPLE, Q, pos_int, Et, 2 * k, SC, cu(cand), cnt[0], cnt[1])
    rows = np.arange(2 * B)[:, None]
    np.testing.assert_array_equal(cnt[0].cpu().numpy(), (c[rows, cand] > p[:, None]).sum(1))
    np.testing.assert_array_equal(cnt[1].cpu().numpy(), (c[rows, cand] == p[:, None]).sum(1))
    assert int(cnt[1].min()) >= 1


@pytest.mark.parametrize("top_n", [1, 10, 128])
def test_topn_equals_a_host_sort_of_the_chain(top_n):
    L, D = _libs()
    k = 37
    Q, _, Et, _, S, *_ = _chain_case(k)
    want_i, want_s = ref.topn_host(S, np.arange(N_ENT), top_n)
    got_i, got_s = D.eval_topn(L.SIMPLE, Q, Et, 2 * k, SC, top_n)
    np.testing.assert_array_equal(got_i.cpu().numpy(), want_i)
    np.testing.assert_array_equal(got_s.cpu().numpy(), want_s)


def test_grid_counts():
    L, D = _libs()
    k = 37
    Q, _, Et, _, S, *_ = _chain_case(k)
    c = ref.cmp_int(S).astype(np.int64)
    thr = np.array([0, 7, 129, 299, 7], np.int32)
    gt, eq = D.eval_grid_count(L.SIMPLE, Q, Et, 2 * k, SC, cu(thr))
    np.testing.assert_array_equal(gt.cpu().numpy(), (c[:, None, :] > c[:, thr, None]).sum(2))
    np.testing.assert_array_equal(eq.cpu().numpy(), (c[:, None, :] == c[:, thr, None]).sum(2))
    gt_h, eq_h = D.eval_grid_count(L.HOLE, Q, Et, 2 * k, SC, cu(thr))
    assert torch.equal(gt, gt_h) and torch.equal(eq, eq_h)


def test_bf16_count_equals_the_hole_call():
    L, D = _libs()
    k = 37
    ki = 2 * k
    Q, _, Et, _, S, tgt, E, R, X = _chain_case(k)
    ld = D.bf16_ld(ki)
    Eb, Qb = D.to_bf16(Et, ki, ld_dst=ld), D.to_bf16(Q, ki, ld_dst=ld)
    out = {}
    for name, mid in (("SimplE", L.SIMPLE), ("HolE", L.HOLE)):
        pos_int, self_ent = D.eval_pos_int_bf16(mid, Eb, ki, SC, cu(X), L.EVAL_S_O, Qb)
        cnt = torch.zeros((2, 2 * B), dtype=torch.int32, device="cuda")
        D.eval_count_bf16(mid, Qb, pos_int, self_ent, Eb, ki, SC, cnt[0], cnt[1])
        out[name] = (pos_int, cnt)
    assert torch.equal(out["SimplE"][0], out["HolE"][0]) and torch.equal(out["SimplE"][1], out["HolE"][1])
    assert int(out["SimplE"][1][0].sum()) > 0 and int(out["SimplE"][1][1].min()) >= 1


# ---- 4. the exact-fast mode --------------------------------------------------------------------------------------------------------
def _fast_case(k, n_ent=5000, nq=130):
    rs = np.random.RandomState(k)
    E = (rs.randn(n_ent, 2 * k) * 0.1).astype(F32)
    R = (rs.randn(4, 2 * k) * 0.1).astype(F32)
    T = np.stack([rs.randint(0, n_ent, nq), rs.randint(0, 4, nq), rs.randint(0, n_ent, nq)], 1).astype(np.int32)
    for j in range(0, nq, 4):                         # exact ties, as the ComplEx precision-2 tests plant them: copies of the true rows
        E[rs.randint(0, n_ent, 2)] = E[T[j, 2]]
        E[rs.randint(0, n_ent, 1)] = E[T[j, 0]]
    F = np.concatenate([T, np.stack([rs.randint(0, n_ent, 5000), rs.randint(0, 4, 5000), rs.randint(0, n_ent, 5000)], 1)]).astype(np.int32)
    return E, R, T, F


@pytest.mark.parametrize("k", [20, 100])
def test_exact_fast_ranks_equal_exact_ranks(k):
    """precision 2 (half-precision prefilter with proven bands, exact re-scoring of the undecided pairs) == precision 0, both sides,
    with a filter; the prefilter decided some candidates and left some undecided, no tile fell back to the exact kernel"""
    L, D = _libs()
    from emgraph_amd.evaluation import rank_triples_device
    E, R, T, F = _fast_case(k)
    Et, Rt = table(E), table(R)
    st = {}
    exact = rank_triples_device(L.SIMPLE, Et, Rt, 2 * k, SC, T, "s,o", "worst", filter_triples=F, precision=0)
    fast = rank_triples_device(L.SIMPLE, Et, Rt, 2 * k, SC, T, "s,o", "worst", filter_triples=F, precision=2, stats=st)
    print("k=%d: stats %r" % (k, st))
    np.testing.assert_array_equal(fast, exact)
    assert st.get("fallback", 0) == 0 and 0 < st["pairs"] < 2 * len(T) * E.shape[0], st
    for side, strategy in (("o", "best"), ("s", "middle")):
        np.testing.assert_array_equal(rank_triples_device(L.SIMPLE, Et, Rt, 2 * k, SC, T, side, strategy, filter_triples=F, precision=2),
                                      rank_triples_device(L.SIMPLE, Et, Rt, 2 * k, SC, T, side, strategy, filter_triples=F, precision=0))


def test_exact_fast_through_tanh():
    L, D = _libs()
    from emgraph_amd.evaluation import rank_triples_device
    from emgraph_amd.evaluation.ranking import link_prefilter_applies
    assert link_prefilter_applies(L.SIMPLE, L.LINK_TANH)
    E, R, T, F = _fast_case(100)
    Et, Rt = table(E), table(R)
    st = {}
    exact = rank_triples_device(L.SIMPLE, Et, Rt, 200, SC, T, "s,o", "worst", filter_triples=F, precision=0, link=L.LINK_TANH)
    fast = rank_triples_device(L.SIMPLE, Et, Rt, 200, SC, T, "s,o", "worst", filter_triples=F, precision=2, link=L.LINK_TANH, stats=st)
    print("tanh: stats %r" % (st,))
    np.testing.assert_array_equal(fast, exact)
    assert not st.get("link_exact_only", False)


# ---- 5. the relation side --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [5, 37, 64])
@pytest.mark.parametrize("n_rel", [3, 70])
def test_relation_side_equals_the_object_side(k, n_rel):
    """one triple, one score: emg_eval_rel_scores_dense has the bits of the object-side emg_eval_scores_dense on the expanded triples
    (s_i, r, o_i); counters and top-N follow on the host from those bits"""
    L, D = _libs()
    ki = 2 * k
    rs = np.random.RandomState(10 * k + n_rel)
    E = (rs.randn(100, ki) * 0.3).astype(F32)
    R = (rs.randn(n_rel, ki) * 0.3).astype(F32)
    T = np.stack([rs.randint(0, 100, 130), rs.randint(0, n_rel, 130), rs.randint(0, 100, 130)], 1).astype(np.int32)
    T[0, 2] = T[0, 0]
    for aligned in (True, False):
        Et, Rt = table(E, None if aligned else ki + 1), table(R, None if aligned else ki + 3)
        cands = np.arange(n_rel)
        Xp = relref.expand(T[:, 0], T[:, 2], cands)
        Q, _ = D.eval_build_queries(L.SIMPLE, Et, Rt, ki, SC, cu(Xp), L.EVAL_O)
        objs = np.unique(T[:, 2].astype(np.int64))
        S_all = D.eval_scores_dense(L.SIMPLE, Q, Et, ki, SC, cand=cu(objs.astype(np.int32))).cpu().numpy()
        S_want = relref.pick_objects(S_all, T[:, 2], n_rel, objs)
        _, pos = D.eval_build_queries(L.SIMPLE, Et, Rt, ki, SC, cu(T), L.EVAL_O)
        S_got = D.eval_rel_scores_dense(L.SIMPLE, Et, Rt, ki, SC, cu(T))
        np.testing.assert_array_equal(S_got.cpu().numpy().view(np.int32), np.ascontiguousarray(S_want, F32).view(np.int32))
        C, pos_h = relref.cmp_int(S_want), pos.cpu().numpy()
        np.testing.assert_array_equal(C[np.arange(len(T)), T[:, 1]], pos_h)
        excl = [sorted(set(rs.choice(n_rel, rs.randint(0, 3), replace=False).tolist()) | {int(p)}) for p in T[:, 1]]
        ptr = np.zeros(len(T) + 1, np.int64)
        ptr[1:] = np.cumsum([len(e) for e in excl])
        idx = np.concatenate([np.asarray(e, np.int32) for e in excl])
        cnt = D.eval_rel_count(L.SIMPLE, Et, Rt, ki, SC, cu(T), pos, excl_ptr=cu(ptr), excl_idx=cu(idx)).cpu().numpy()
        for got, want in zip(cnt, relref.counts(C, pos_h, cands, excl)):
            np.testing.assert_array_equal(got, want)
        for top_n in (1, 10):
            want_i, want_s = relref.host_topn(S_want, cands, top_n, excl)
            got_i, got_s = D.eval_rel_topn(S_got, top_n, excl_ptr=cu(ptr), excl_idx=cu(idx))
            np.testing.assert_array_equal(got_i.cpu().numpy(), want_i)
            np.testing.assert_array_equal(got_s.cpu().numpy().view(np.int32), want_s)


# ---- 6. training -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,eta", [(5, 2), (37, 5), (200, 2), (65, 82)])
def test_one_sgd_step_moves_the_tables_by_the_reference_gradient(k, eta):
    """pairwise loss with a margin no pair reaches: dL/df_neg = 1 per negative, dL/df_pos = -eta.  The tables move by -lr times the float64
    gradient within lr times the gradient bound of test 1 — and what a float32 TABLE adds to a gradient row, neither of which the
    gradient bound can hold: the apply adds the m slots of a destination (m - 1 roundings of partial sums, each at most the sum of
    |terms|) and multiplies by lr (one more), and the stored value E - lr G is rounded once, 2^-24 |E1|:
        |(E1 - E) + lr G64| <= lr (eta + 4 + m) 2^-24 sum|terms| + 2^-24 |E1|
    The worst ratio to this bound and to lr times the gradient bound alone are printed.  Measured on one MI355X: 0.90 / 0.95 / 0.98 /
    0.11 of the bound for the entity table at (k, eta) = (5, 2) / (37, 5) / (200, 2) / (65, 82) and 0.08 / 0.09 / 0.16 / 0.03 for the
    relation table.  lr times the gradient bound ALONE holds for the relation table (0.33 / 0.26 / 0.75 / 0.03) and for the entity table
    at eta = 82 (0.18), and cannot hold for an entity row that few small terms feed: there the stored value's own rounding, 2^-24 |E1|,
    is 4e4 .. 3e6 times lr times the gradient bound — a property of float32 storage, not of the gradient."""
    L, D = _libs()
    from emgraph_amd.training import Trainer
    E, R, X, codes, xneg, keep_s, repl = _case(k, eta)
    ki, lr = 2 * k, 0.05
    tr = Trainer(L.SIMPLE, ki, SC, E, R, eta, loss="pairwise", loss_params={"margin": 1e4}, optimizer="sgd", optimizer_params={"lr": lr},
                 batches_count=1, seed=5)
    assert tr.generic and not tr.fused and not tr.inplace and not tr.factored
    tr.set_training_set(X, B)
    tr.step(0, B, epoch=1, batch=1, inj_mask=cu(keep_s), inj_repl=cu(repl))
    E1, R1 = tr.tables_numpy()
    T, g = np.concatenate([X, xneg]), np.concatenate([np.full(B, -float(eta)), np.ones(B * eta)])
    eE, eR = ref.grads_f64(E, R, T, g)
    tE, tR = ref.grad_terms_f64(E, R, T, g)
    mE = (np.bincount(T[:, 0], minlength=N_ENT) + np.bincount(T[:, 2], minlength=N_ENT))[:, None]
    mR = np.bincount(X[:, 1], minlength=N_REL)[:, None]
    for name, W0, W1, eW, tW, m in (("ent", E, E1, eE, tE, mE), ("rel", R, R1, eR, tR, mR)):
        err = np.abs((W1.astype(np.float64) - W0) + lr * eW)
        bound = lr * (eta + 4 + m) * ref.U * tW + ref.U * np.abs(W1)
        lit = lr * (eta + 4) * ref.U * tW
        print("k=%d eta=%d %s: worst error %.3f of the bound, %.3f of lr x the gradient bound alone" % (
            k, eta, name, (err[bound > 0] / bound[bound > 0]).max(), (err[lit > 0] / lit[lit > 0]).max()))
        assert np.all(err <= bound)
        assert np.all(W1[tW == 0] == W0[tW == 0]) and np.abs(W1 - W0).max() > 0


@pytest.mark.parametrize("loss,opt", [("self_adversarial", "adam"), ("multiclass_nll", "sgd")])
def test_train_step_one_call_simple(loss, opt):
    """emg_train_step with EMG_SIMPLE: the generic unfused step — the same tables as the Trainer's step, three batches"""
    L, D = _libs()
    from emgraph_amd.training import Trainer
    k, n_ent, n_rel, Bs, eta = 10, 300, 6, 128, 3
    ki = 2 * k
    rs = np.random.RandomState(3)
    E = rs.uniform(-0.5, 0.5, (n_ent, ki)).astype(F32)
    R = rs.uniform(-0.5, 0.5, (n_rel, ki)).astype(F32)
    X = np.stack([rs.randint(0, n_ent, 3 * Bs), rs.randint(0, n_rel, 3 * Bs), rs.randint(0, n_ent, 3 * Bs)], 1).astype(np.int32)
    mk = lambda: Trainer(L.SIMPLE, ki, SC, E, R, eta, loss=loss, optimizer=opt, optimizer_params={"lr": 0.05}, batches_count=3, seed=5)  # noqa: E731
    tr, tr2 = mk(), mk()
    tr.set_training_set(X, Bs)
    assert tr.generic and not tr.fused and not tr.inplace
    ws = torch.empty(D.train_step_workspace_bytes(Bs, eta, ki, n_ent, n_rel), dtype=torch.uint8, device="cuda")
    Xt = cu(X)
    for b in range(3):
        tr.step(b * Bs, Bs, epoch=1, batch=b + 1)
        tr2.step_count += 1
        D.train_step(L.SIMPLE, tr2.ent, tr2.rel, ki, SC, Xt[b * Bs:(b + 1) * Bs], eta, tr2.sides, tr2.loss_id, tr2.loss_accum[0:1],
                     tr2.opt_id, tr2.step_count, tr2._hyper(tr2.lr), ws, margin=tr2.margin, alpha=tr2.alpha,
                     states=(tr2.state_ent[0], tr2.state_ent[1], tr2.state_rel[0], tr2.state_rel[1]),
                     tags=(tr2.tag_ent, tr2.tag_rel), n_choices=n_ent, seed=5, counter0=b, inplace=True)   # (inplace is ignored for this model)
    torch.cuda.synchronize()
    tr.materialize()
    assert torch.equal(tr.ent, tr2.ent) and torch.equal(tr.rel, tr2.rel)
    assert not torch.equal(tr.ent[:, :ki].cpu(), torch.from_numpy(E))
    assert tr.read_loss() == pytest.approx(tr2.read_loss(), rel=1e-12)


# ---- 7. refusals on the device -------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device():
    L, D = _libs()
    E, R, X, codes, _, _, _ = _case(5, 2)
    Et, Rt, Xt = table(E), table(R), cu(X)
    with pytest.raises(L.EmgError, match="EMG_SIMPLE"):
        D.score_triples(L.SIMPLE, Et, Rt, 9, SC, Xt)
    with pytest.raises(L.EmgError, match="EMG_SIMPLE"):
        D.train_forward(L.SIMPLE, Et, Rt, 9, SC, Xt, 2, cu(codes))
    with pytest.raises(L.EmgError, match="EMG_SIMPLE"):
        D.eval_build_queries(L.SIMPLE, Et, Rt, 9, SC, Xt, L.EVAL_O)
    with pytest.raises(L.EmgError, match="EMG_SIMPLE"):
        D.eval_rel_scores_dense(L.SIMPLE, Et, Rt, 9, SC, Xt)
    with pytest.raises(L.EmgError, match="unknown model"):
        D.score_triples(7, Et, Rt, 10, SC, Xt)
    with pytest.raises(L.EmgError, match="unknown model"):
        D.eval_build_queries(7, Et, Rt, 10, SC, Xt, L.EVAL_O)
    with pytest.raises(L.EmgError, match="unknown model"):
        D.shared_forward(L.SIMPLE, Et, Rt, 10, SC, Xt, 16, 2, torch.zeros(2 * ((B + 15) // 16), dtype=torch.int32, device="cuda"))
    sp = D.score_triples(L.SIMPLE, Et, Rt, 10, SC, Xt)
    state = torch.zeros(8, dtype=torch.float64, device="cuda")
    with pytest.raises(L.EmgError, match="unknown model"):
        D.calib_step(L.SIMPLE, Et, Rt, 10, SC, Xt, sp, 0, 0, 1.0, 0.0, 1.0, 1.0, state, D.calib_workspace(B, Et.device))


# ---- 8. the public API -------------------------------------------------------------------------------------------------------------
N_RING = 60


def _ring():
    ents = np.array(["n%02d" % i for i in range(N_RING)])
    nxt = np.stack([ents, np.full(N_RING, "next"), np.roll(ents, -1)], 1)
    prv = np.stack([np.roll(ents, -1), np.full(N_RING, "prev"), ents], 1)
    return np.concatenate([nxt, prv])


def _ring_model(**kw):
    from emgraph_amd.models import SimplE
    args = dict(k=8, eta=3, epochs=20, batches_count=2, seed=7, loss="self_adversarial", optimizer="adam", optimizer_params={"lr": 0.05},
                embedding_model_params={"eval_precision": "auto"})
    args.update(kw)
    return SimplE(**args)


def test_public_api_on_a_ring(tmp_path):
    L, D = _libs()
    from emgraph_amd.discovery import discover_facts, find_nearest_neighbours
    from emgraph_amd.evaluation import evaluate_performance, evaluate_relation_prediction
    from emgraph_amd.evaluation.protocol import topn_completions
    from emgraph_amd.evaluation.ranking import FilterIndex, ranks_from_counts
    from emgraph_amd.utils import restore_model, save_model
    X = _ring()
    m = _ring_model()
    m.fit(X)
    assert m.epoch_losses[-1] < m.epoch_losses[0]
    E, R = (np.asarray(a, F32) for a in m.trained_model_params[:2])
    assert E.shape == (N_RING, 16) and R.shape == (2, 16) and np.abs(R[:, 8:]).max() > 0
    assert m.get_embeddings(["next", "prev"], "relation").shape == (2, 16)
    Xi = np.stack([[m.ent_to_idx[s] for s in X[:, 0]], [m.rel_to_idx[r] for r in X[:, 1]], [m.ent_to_idx[o] for o in X[:, 2]]], 1).astype(np.int32)
    # ranks from the C chain on the float32 query rows of the trained tables
    n = len(Xi)
    Q = np.concatenate([ref.queries_f32(E, R, Xi, True), ref.queries_f32(E, R, Xi, False)])
    S = ref.chain_f32(Q, E)
    c, p = ref.cmp_int(S), ref.cmp_int(S[np.arange(2 * n), np.concatenate([Xi[:, 2], Xi[:, 0]])])
    ptr, idx = FilterIndex(Xi).csr(Xi, L.EVAL_S_O, N_RING)
    fgt = np.array([(c[r, idx[ptr[r]:ptr[r + 1]]] > p[r]).sum() for r in range(2 * n)])
    feq = np.array([(c[r, idx[ptr[r]:ptr[r + 1]]] == p[r]).sum() for r in range(2 * n)])
    want = ranks_from_counts((c > p[:, None]).sum(1), (c == p[:, None]).sum(1), fgt, feq, n, "s,o", "worst")
    for prec in ("auto", 0, 2):
        m.embedding_model_params["eval_precision"] = prec
        got = np.asarray(evaluate_performance(X, m, filter_triples=X))            # (model.get_ranks on an adapter)
        np.testing.assert_array_equal(got.reshape(want.shape), want, err_msg=str(prec))
        np.testing.assert_array_equal(m.get_ranks_idx(Xi, filter_idx=FilterIndex(Xi)), want, err_msg=str(prec))
    m.embedding_model_params["eval_precision"] = "auto"
    # predict, top-N, calibration, save / restore
    scores = m.predict(X)
    assert np.all(np.abs(scores.astype(np.float64) - ref.score_f64(E, R, Xi)) <= ref.score_bound(E, R, Xi))
    ents, sc = topn_completions(X[:5, :2], m, side="o", top_n=3)
    assert ents.shape == (5, 3) and np.all(np.diff(sc, axis=1) <= 0)
    neg = X.copy()
    neg[:, 2] = np.roll(X[:, 2], 7)
    m.calibrate(X, X_neg=neg)
    proba = m.predict_proba(X)
    assert proba.shape == (len(X),) and np.all((proba >= 0) & (proba <= 1))
    with pytest.raises(NotImplementedError, match="SimplE"):
        m.calibrate(X, positive_base_rate=0.5)
    path = str(tmp_path / "simple.pkl")
    save_model(m, path)
    m2 = restore_model(path)
    assert type(m2).__name__ == "SimplE"
    np.testing.assert_array_equal(m2.predict(X), scores)
    np.testing.assert_array_equal(m2.predict_proba(X), proba)
    # discovery and the relation side
    found, ranks = discover_facts(X, m, top_n=N_RING, strategy="exhaustive")
    known = set(map(tuple, X.astype(str)))
    assert len(found) > 0 and found.shape[1] == 3 and len(ranks) == len(found) and not (set(map(tuple, found.astype(str))) & known)
    nb, dist = find_nearest_neighbours(m, entities=["n00", "n01"], n_neighbors=3)
    assert np.asarray(nb).shape == (2, 3)
    rr = np.asarray(evaluate_relation_prediction(X[:40], m, filter_triples=X))
    assert rr.shape == (40,) and rr.min() >= 1


def test_rank_through_link_regulariser_and_early_stopping():
    from emgraph_amd.evaluation import evaluate_performance
    X = _ring()
    m = _ring_model(epochs=30, loss="nll", optimizer="sgd", optimizer_params={"lr": 1e-12}, regularizer="LP",
                    regularizer_params={"p": 2, "lambda": 1e-5},
                    embedding_model_params={"non_linearity": "tanh", "rank_through_link": True})
    m.fit(X, early_stopping=True, early_stopping_params={"x_valid": X[:32], "criteria": "mrr", "burn_in": 0, "check_interval": 1,
                                                         "stop_interval": 2, "x_filter": X})
    assert m.is_fitted and m.early_stopping_epoch is not None and m.early_stopping_epoch <= 4   # (a rate too small to move a rank)
    ranks = np.asarray(evaluate_performance(X[:16], m, filter_triples=X))
    assert ranks.shape == (16, 2) and ranks.min() >= 1
