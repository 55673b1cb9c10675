"""RotatE (EMG_ROTATE) on the device against the host references of tests/_rotate_ref.py: scores and gradients of the generic
training kernels against float64, the query rows against float64, every 1-vs-all kernel (dense, count, filter, top-N) against
the float32 restatement of the canonical chain TO THE BIT, one optimizer step, and the public API.

Shapes (tests/_rotate_ref.py: 130 entities, 70 positives / query rows, 5 relations): two candidate tiles of 64 and a tail, a
second block of 64 rows with a tail; k = 5 (k_int = 10: narrower than a k-tile, no multiple of 4), 37 (a k-tile of 16
coordinates twice plus a tail), 64 (whole tiles).

The training kernels (csrc/emg_score.hip: rotate_forward_kernel, rotate_backward_kernel, score_rotate_kernel; lane l owns the complex
coordinates l, l + 64, ...; (cos, sin) cached in LDS below coordinate 512) also at the widths of WIDE: k = 65 (lane 0 owns two
coordinates, the others one), 100 and 200 (the widths in use), 128 (whole trips), 513 and 520 (one / eight coordinates past the
phase cache: sincosf per triple), 640 with phases of +-20 (the uncached branch with sincosf's argument reduction); the query, dense
and count kernels also at k = 200 (twelve whole k-tiles and a tail of eight); the generic step at k = 200 and 513 (k_int = 1026:
wider than 1024, no multiple of 4) and with eta = 82 > 64 negatives per positive."""
import functools

import numpy as np
import pytest

from tests import _rotate_ref as ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32 = np.float32
KS = (5, 37, 64)
ETAS = (2, 5)
# (k, eta, phase) past one coordinate per lane — the combinations of these widths whose training_case is well conditioned
# (tests/test_rotate_host.py::test_device_cases_are_well_conditioned)
WIDE = [(65, 2, np.pi), (65, 5, np.pi), (100, 5, np.pi), (128, 2, np.pi), (200, 2, np.pi), (513, 2, np.pi), (513, 5, np.pi), (520, 5, np.pi),
        (100, 5, 20.0), (128, 2, 20.0), (200, 2, 20.0), (200, 5, 20.0), (640, 2, 20.0)]
ETA_WIDE = 82                  # more negatives than lanes; the nearest eta >= 65 whose case at k = 65 is well conditioned
N_ENT, N_REL, B = ref.N_ENT, ref.N_REL, ref.N_POS


def _libs():
    from emgraph_amd import _lib as L
    from emgraph_amd import device as D
    D.require_gpu()
    return L, D


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def table(a, ld=None):
    """a device table holding ``a``: row stride padded to 16 bytes, or ``ld`` floats (an odd one: rows of no alignment)"""
    n, k = a.shape
    buf = torch.zeros((n, ld or ((k + 3) // 4) * 4), dtype=torch.float32, device="cuda")
    buf[:, :k] = cu(a)
    return buf[:, :k]


@functools.lru_cache(maxsize=None)
def _case(k, eta, phase=np.pi):
    case = ref.training_case(k, eta, phase)
    assert ref.well_conditioned(case[0], case[1], case[2], case[4])       # (a condition of the comparison, checked on the reference)
    return case


# ---- 1, 2. the generic training kernels against float64 --------------------------------------------------------------------------
@pytest.mark.parametrize("k,eta,phase", [(k, eta, np.pi) for k in KS for eta in ETAS] + [(37, 2, 20.0)] + WIDE)
def test_scores_and_gradients_vs_float64(k, eta, phase):
    """scores rtol 1e-4 / atol 1e-6, gradient rows rtol 1e-4 / atol 1e-5 max|grad|: the bars of the other generic model
    (test_transe_any_norm_forward_backward_vs_oracle).  phase 20: sincosf reduces its argument.  The planted triple (a, 4, a) with
    relation 4 = 0 has d = 0 in every coordinate: score -0 / +0, and — its negatives' upstream gradients set to 0 — rows of zeros.
    score_triples takes sincosf per triple, train_forward reads the group's cache below coordinate 512 and takes it per triple
    from there on: the same bits at every width."""
    L, D = _libs()
    E, R, X, codes, xneg, _, _ = _case(k, eta, phase)
    ki = 2 * k
    Et, Rt, Xt, ct = table(E), table(R), cu(X), cu(codes)
    sp, sn = D.train_forward(L.ROTATE, Et, Rt, ki, 1.0, Xt, eta, ct)
    sp, sn = sp.cpu().numpy(), sn.cpu().numpy()
    np.testing.assert_allclose(sp, ref.score_f64(E, R, X), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(sn, ref.score_f64(E, R, xneg), rtol=1e-4, atol=1e-6)
    assert sp[0] == 0.0
    np.testing.assert_array_equal(D.score_triples(L.ROTATE, Et, Rt, ki, 1.0, Xt).cpu().numpy(), sp)

    rs = np.random.RandomState(k + eta)
    gpos = rs.randn(B).astype(F32)
    gneg = rs.randn(B * eta).astype(F32)
    gneg[0::B] = 0.0                                             # the planted group's negatives
    ldc = ((ki + 3) // 4) * 4
    ce = torch.full(((2 + eta) * B, ldc), 7.0, dtype=torch.float32, device="cuda")    # (every slot is written, not accumulated into)
    cr = torch.full((B, ldc), 7.0, dtype=torch.float32, device="cuda")
    de = torch.empty((2 + eta) * B, dtype=torch.int32, device="cuda")
    dr = torch.empty(B, dtype=torch.int32, device="cuda")
    D.train_backward(L.ROTATE, Et, Rt, ki, 1.0, Xt, eta, ct, cu(gpos), cu(gneg), ce, cr, de, dr)
    ce, cr = ce.cpu().numpy()[:, :ki], cr.cpu().numpy()[:, :ki]
    assert np.all(np.isfinite(ce)) and np.all(np.isfinite(cr))
    assert np.all(cr[:, k:] == 0.0)                              # the unused relation columns
    own = np.concatenate([[0, B], 2 * B + B * np.arange(eta)])   # every slot of the planted group
    assert not ce[own].any() and not cr[0].any()
    dE = np.zeros((N_ENT, ki))
    dR = np.zeros((N_REL, ki))
    np.add.at(dE, de.cpu().numpy(), ce.astype(np.float64))
    np.add.at(dR, dr.cpu().numpy(), cr.astype(np.float64))
    eE, eR = ref.grads_f64(E, R, X, gpos)
    a, b = ref.grads_f64(E, R, xneg, gneg)
    eE += a
    eR += b
    print("k=%d eta=%d phase=%.1f: max |dE - ref| = %.3g (max |ref| %.3g), max |dR - ref| = %.3g (max |ref| %.3g)"
          % (k, eta, phase, np.abs(dE - eE).max(), np.abs(eE).max(), np.abs(dR - eR).max(), np.abs(eR).max()))
    np.testing.assert_allclose(dE, eE, rtol=1e-4, atol=1e-5 * np.abs(eE).max())
    np.testing.assert_allclose(dR, eR, rtol=1e-4, atol=1e-5 * np.abs(eR).max())


def test_odd_k_int_and_unsupported_calls_are_refused():
    L, D = _libs()
    E, R, X, codes, _, _, _ = _case(5, 2)
    Et, Rt, Xt = table(E), table(R), cu(X)
    with pytest.raises(L.EmgError, match="EMG_ROTATE"):
        D.score_triples(L.ROTATE, Et, Rt, 9, 1.0, Xt)
    Q, pos_int = D.eval_build_queries(L.ROTATE, Et, Rt, 10, 1.0, Xt, L.EVAL_O)
    cnt = torch.zeros((2, B), dtype=torch.int32, device="cuda")
    for precision in (1, 2):
        with pytest.raises(L.EmgError, match="exact kernel only"):
            D.eval_count(L.ROTATE, Q, pos_int, Et, 10, 1.0, cnt[0], cnt[1], precision=precision)
    with pytest.raises(L.EmgError, match="unknown model"):
        D.eval_grid_count(L.ROTATE, Q, Et, 10, 1.0, torch.zeros(1, dtype=torch.int32, device="cuda"))
    with pytest.raises(L.EmgError, match="unknown model"):
        D.score_triples(7, Et, Rt, 10, 1.0, Xt)


# ---- 3. query rows against float64 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,phase", [(k, np.pi) for k in KS] + [(37, 20.0), (200, np.pi)])
def test_query_rows_vs_float64(k, phase):
    """q = x o r (object side) / x o conj(r) (subject side), x the kept entity: each half is fma(c, x_a, +-(s * x_b)) — cos / sin within
    2 ulp each (sincosf), the product, the fused multiply-add's one rounding: |err| <= 4 * 2^-23 * (|x_re| + |x_im|) per element"""
    L, D = _libs()
    E, R, X, _, _, _, _ = _case(k, 2, phase)
    Q, _ = D.eval_build_queries(L.ROTATE, table(E), table(R), 2 * k, 1.0, cu(X), L.EVAL_S_O)
    Q = Q.cpu().numpy()[:, :2 * k].astype(np.float64)
    worst = 0.0
    for rows, obj in ((Q[:B], True), (Q[B:], False)):
        x = E[X[:, 0] if obj else X[:, 2]].astype(np.float64)
        bound = 4 * 2.0 ** -23 * (np.abs(x[:, :k]) + np.abs(x[:, k:]))
        err = np.abs(rows - ref.queries_f64(E, R, X, obj))
        worst = max(worst, float((err / np.tile(bound, 2)).max()))
        assert np.all(err <= np.tile(bound, 2))
    print("k=%d phase=%.1f: largest error of a query element = %.3f of its bound" % (k, phase, worst))


# ---- 4. the canonical chain, to the bit --------------------------------------------------------------------------------------------
def _chain_case(k, ld=None, ldq=None):
    """(Q device, pos_int device, Et, S host chain from the device's own query rows, tgt)"""
    L, D = _libs()
    E, R, X, _, _, _, _ = _case(k, 2)
    Et, Rt = table(E, ld), table(R)
    Q, pos_int = D.eval_build_queries(L.ROTATE, Et, Rt, 2 * k, 1.0, cu(X), L.EVAL_S_O, ldq=ldq)
    S = ref.chain_f32(Q.cpu().numpy()[:, :2 * k], E)
    tgt = np.concatenate([X[:, 2], X[:, 0]])
    return Q, pos_int, Et, S, tgt, E, R, X


@pytest.mark.parametrize("k", KS + (200,))
@pytest.mark.parametrize("aligned", [True, False])
def test_dense_scores_and_counts_equal_the_host_chain(k, aligned):
    L, D = _libs()
    ki = 2 * k
    Q, pos_int, Et, S, tgt, E, R, X = _chain_case(k, *((None, None) if aligned else (ki + 1, ki + 3)))
    assert (Et.stride(0) % 4 == 0) == aligned
    got = D.eval_scores_dense(L.ROTATE, Q, Et, ki, 1.0).cpu().numpy()
    np.testing.assert_array_equal(got, S)
    assert got[0, ref.PLANT] == 0.0                              # the planted triple: every modulus is 0
    c, p = ref.cmp_int(S), ref.cmp_int(S[np.arange(2 * B), tgt])
    np.testing.assert_array_equal(pos_int.cpu().numpy(), p)
    cnt = torch.zeros((4, 2 * B), dtype=torch.int32, device="cuda")
    D.eval_count(L.ROTATE, Q, pos_int, Et, ki, 1.0, cnt[0], cnt[1])
    np.testing.assert_array_equal(cnt[0].cpu().numpy(), (c > p[:, None]).sum(1))
    np.testing.assert_array_equal(cnt[1].cpu().numpy(), (c == p[:, None]).sum(1))
    # a candidate list (and its dense scores)
    subset = np.unique(np.random.RandomState(k).randint(0, N_ENT, 90)).astype(np.int32)
    cnt.zero_()
    D.eval_count(L.ROTATE, Q, pos_int, Et, ki, 1.0, cnt[0], cnt[1], cand=cu(subset))
    np.testing.assert_array_equal(cnt[0].cpu().numpy(), (c[:, subset] > p[:, None]).sum(1))
    np.testing.assert_array_equal(cnt[1].cpu().numpy(), (c[:, subset] == p[:, None]).sum(1))
    np.testing.assert_array_equal(D.eval_scores_dense(L.ROTATE, Q, Et, ki, 1.0, cand=cu(subset)).cpu().numpy(), S[:, subset])
    # the filter's counters go through chain_score
    from emgraph_amd.evaluation.ranking import FilterIndex
    rs = np.random.RandomState(k + 1)
    F = np.concatenate([X, np.stack([rs.randint(0, N_ENT, 600), rs.randint(0, N_REL, 600), rs.randint(0, N_ENT, 600)], 1)]).astype(np.int32)
    ptr, idx = FilterIndex(F).csr(X, L.EVAL_S_O, N_ENT)
    D.eval_filter_count(L.ROTATE, Q, pos_int, Et, 0, ki, 1.0, cu(ptr), cu(idx), cnt[2], cnt[3])
    np.testing.assert_array_equal(cnt[2].cpu().numpy(), [(c[r, idx[ptr[r]:ptr[r + 1]]] > p[r]).sum() for r in range(2 * B)])
    np.testing.assert_array_equal(cnt[3].cpu().numpy(), [(c[r, idx[ptr[r]:ptr[r + 1]]] == p[r]).sum() for r in range(2 * B)])


@pytest.mark.parametrize("k", KS)
def test_counts_and_ranks_through_tanh(k):
    """the LINKED compare epilogue: the integers are int32(tanh(score) * 1e5) with the device's tanh bits (emg_link_scores) of the
    host chain's scores"""
    L, D = _libs()
    from emgraph_amd.evaluation import rank_triples_device
    from emgraph_amd.evaluation.ranking import FilterIndex, ranks_from_counts
    ki = 2 * k
    Q, _, Et, S, tgt, E, R, X = _chain_case(k)
    E = E.copy()
    neg = cu(S.reshape(-1))
    pos = cu(S[np.arange(2 * B), tgt])
    D.link_scores(L.LINK_TANH, None, 0.0, pos, neg, 2 * B, N_ENT)
    c, p = ref.cmp_int(neg.cpu().numpy().reshape(2 * B, N_ENT)), ref.cmp_int(pos.cpu().numpy())
    Rt = table(R)
    Q2, pos_int = D.eval_build_queries(L.ROTATE, Et, Rt, ki, 1.0, cu(X), L.EVAL_S_O, link=L.LINK_TANH)
    assert torch.equal(Q2, Q)
    np.testing.assert_array_equal(pos_int.cpu().numpy(), p)
    cnt = torch.zeros((2, 2 * B), dtype=torch.int32, device="cuda")
    D.eval_count(L.ROTATE, Q, pos_int, Et, ki, 1.0, cnt[0], cnt[1], link=L.LINK_TANH)
    gt, eq = (c > p[:, None]).sum(1), (c == p[:, None]).sum(1)
    np.testing.assert_array_equal(cnt[0].cpu().numpy(), gt)
    np.testing.assert_array_equal(cnt[1].cpu().numpy(), eq)
    assert eq.min() >= 1
    ptr, idx = FilterIndex(X).csr(X, L.EVAL_S_O, N_ENT)
    fgt = np.array([(c[r, idx[ptr[r]:ptr[r + 1]]] > p[r]).sum() for r in range(2 * B)])
    feq = np.array([(c[r, idx[ptr[r]:ptr[r + 1]]] == p[r]).sum() for r in range(2 * B)])
    want = ranks_from_counts(gt, eq, fgt, feq, B, "s,o", "worst")
    got = rank_triples_device(L.ROTATE, Et, Rt, ki, 1.0, X, "s,o", "worst", filter_triples=X, link=L.LINK_TANH)
    np.testing.assert_array_equal(got, want)


# ---- 5. top-N ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("top_n", [1, 10, 128])
def test_topn_equals_a_host_sort_of_the_chain(k, top_n):
    L, D = _libs()
    from emgraph_amd.evaluation.ranking import topn_device
    ki = 2 * k
    Q, _, Et, S, _, E, R, X = _chain_case(k)
    Rt = table(R)
    rs = np.random.RandomState(k + 2)
    F = np.concatenate([X, np.stack([X[rs.randint(0, B, 900), 0], X[rs.randint(0, B, 900), 1], rs.randint(0, N_ENT, 900)], 1),
                        np.stack([rs.randint(0, N_ENT, 900), X[rs.randint(0, B, 900), 1], X[rs.randint(0, B, 900), 2]], 1)]).astype(np.int32)
    subset = np.unique(rs.randint(0, N_ENT, 90)).astype(np.int32)
    for side, rows, qcols in (("o", S[:B], (0, 1)), ("s", S[B:], (1, 2))):
        queries = X[:, qcols]
        if side == "o":
            known = [np.unique(F[(F[:, 0] == s) & (F[:, 1] == p_), 2]) for s, p_ in queries]
        else:
            known = [np.unique(F[(F[:, 1] == p_) & (F[:, 2] == o), 0]) for p_, o in queries]
        assert max(len(x) for x in known) > 1
        for sub in (None, subset):
            ids = np.arange(N_ENT) if sub is None else sub
            want_i, want_s = ref.topn_host(rows[:, ids], ids, top_n, known)
            got_i, got_s = topn_device(L.ROTATE, Et, Rt, ki, 1.0, queries, side, top_n, filter_triples=F, entities_subset=sub)
            np.testing.assert_array_equal(got_i, want_i, err_msg=str((side, sub is not None)))
            np.testing.assert_array_equal(got_s, want_s, err_msg=str((side, sub is not None)))


# ---- 6. one step -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,eta", [(5, 2), (37, 5), (200, 2), (513, 2), (65, ETA_WIDE)])
def test_one_sgd_step_moves_the_tables_by_the_reference_gradient(k, eta):
    """pairwise loss with a margin no pair reaches: dL/df_neg = 1 per negative, dL/df_pos = -eta — the step is -lr times the float64
    gradient, within the gradient tolerance times lr (float32 rounding of the update: 2^-24 * 0.5, far below it).  (65, 82): the
    eta-major codes and scores with more negatives than lanes, 82 terms accumulated into a slot."""
    L, D = _libs()
    from emgraph_amd.training import Trainer
    E, R, X, codes, xneg, keep_s, repl = _case(k, eta)
    ki, lr = 2 * k, 0.05
    tr = Trainer(L.ROTATE, ki, 1.0, E, R, eta, loss="pairwise", loss_params={"margin": 1e4}, optimizer="sgd", optimizer_params={"lr": lr},
                 batches_count=1, seed=5)
    assert tr.generic and not tr.fused and not tr.inplace and not tr.factored
    tr.set_training_set(X, B)
    tr.step(0, B, epoch=1, batch=1, inj_mask=cu(keep_s), inj_repl=cu(repl))
    E1, R1 = tr.tables_numpy()
    eE, eR = ref.grads_f64(E, R, X, np.full(B, -float(eta)))
    a, b = ref.grads_f64(E, R, xneg, np.ones(B * eta))
    eE += a
    eR += b
    np.testing.assert_allclose(E1.astype(np.float64) - E, -lr * eE, rtol=1e-4, atol=lr * 1e-5 * np.abs(eE).max())
    np.testing.assert_allclose(R1.astype(np.float64) - R, -lr * eR, rtol=1e-4, atol=lr * 1e-5 * np.abs(eR).max())
    assert np.all(R1[:, k:] == 0.0) and np.abs(R1 - R).max() > 0


@pytest.mark.parametrize("loss,opt", [("self_adversarial", "adam"), ("multiclass_nll", "sgd")])
def test_train_step_one_call_rotate(loss, opt):
    """emg_train_step with EMG_ROTATE: the generic unfused step — the same tables as the Trainer's step (emg_plan_step), three batches"""
    L, D = _libs()
    from emgraph_amd.training import Trainer
    k, n_ent, n_rel, Bs, eta = 10, 300, 6, 128, 3
    ki = 2 * k
    rs = np.random.RandomState(3)
    E = rs.uniform(-0.5, 0.5, (n_ent, ki)).astype(F32)
    R = np.zeros((n_rel, ki), F32)
    R[:, :k] = rs.uniform(-np.pi, np.pi, (n_rel, k))
    X = np.stack([rs.randint(0, n_ent, 3 * Bs), rs.randint(0, n_rel, 3 * Bs), rs.randint(0, n_ent, 3 * Bs)], 1).astype(np.int32)
    mk = lambda: Trainer(L.ROTATE, ki, 1.0, E, R, eta, loss=loss, optimizer=opt, optimizer_params={"lr": 0.05}, batches_count=3, seed=5)  # noqa: E731
    tr, tr2 = mk(), mk()
    tr.set_training_set(X, Bs)
    assert tr.generic and not tr.fused and not tr.inplace
    ws = torch.empty(D.train_step_workspace_bytes(Bs, eta, ki, n_ent, n_rel), dtype=torch.uint8, device="cuda")
    Xt = cu(X)
    for b in range(3):
        tr.step(b * Bs, Bs, epoch=1, batch=b + 1)
        tr2.step_count += 1
        D.train_step(L.ROTATE, tr2.ent, tr2.rel, ki, 1.0, Xt[b * Bs:(b + 1) * Bs], eta, tr2.sides, tr2.loss_id, tr2.loss_accum[0:1],
                     tr2.opt_id, tr2.step_count, tr2._hyper(tr2.lr), ws, margin=tr2.margin, alpha=tr2.alpha,
                     states=(tr2.state_ent[0], tr2.state_ent[1], tr2.state_rel[0], tr2.state_rel[1]),
                     tags=(tr2.tag_ent, tr2.tag_rel), n_choices=n_ent, seed=5, counter0=b, inplace=True)   # (inplace is ignored for this model)
    torch.cuda.synchronize()
    tr.materialize()
    assert torch.equal(tr.ent, tr2.ent) and torch.equal(tr.rel, tr2.rel)
    assert not torch.equal(tr.ent[:, :ki].cpu(), torch.from_numpy(E))
    assert torch.all(tr.rel[:, k:ki] == 0)
    assert tr.read_loss() == pytest.approx(tr2.read_loss(), rel=1e-12)


# ---- 7. the public API -------------------------------------------------------------------------------------------------------------
N_RING = 60


def _ring():
    ents = np.array(["n%02d" % i for i in range(N_RING)])
    nxt = np.stack([ents, np.full(N_RING, "next"), np.roll(ents, -1)], 1)
    prv = np.stack([np.roll(ents, -1), np.full(N_RING, "prev"), ents], 1)
    return np.concatenate([nxt, prv])


def _ring_model(**kw):
    from emgraph_amd.models import RotatE
    args = dict(k=8, eta=3, epochs=20, batches_count=2, seed=7, loss="self_adversarial", optimizer="adam", optimizer_params={"lr": 0.05},
                embedding_model_params={"eval_precision": "auto"})
    args.update(kw)
    return RotatE(**args)


def test_public_api_on_a_ring(tmp_path):
    L, D = _libs()
    from emgraph_amd.evaluation import evaluate_performance
    from emgraph_amd.evaluation.protocol import topn_completions
    from emgraph_amd.evaluation.ranking import FilterIndex, ranks_from_counts
    from emgraph_amd.utils import restore_model, save_model
    X = _ring()
    m = _ring_model()
    m.fit(X)
    assert m.epoch_losses[-1] < m.epoch_losses[0]
    E, R = (np.asarray(a, F32) for a in m.trained_model_params[:2])
    assert E.shape == (N_RING, 16) and R.shape == (2, 16) and not R[:, 8:].any()
    assert m.get_embeddings(["next", "prev"], "relation").shape == (2, 8)
    Xi = np.stack([[m.ent_to_idx[s] for s in X[:, 0]], [m.rel_to_idx[r] for r in X[:, 1]], [m.ent_to_idx[o] for o in X[:, 2]]], 1).astype(np.int32)
    # ranks from the host chain on the model's tables (the device's query rows)
    Et, Rt = table(E), table(R)
    Q, _ = D.eval_build_queries(L.ROTATE, Et, Rt, 16, 1.0, cu(Xi), L.EVAL_S_O)
    S = ref.chain_f32(Q.cpu().numpy()[:, :16], E)
    n = len(Xi)
    c, p = ref.cmp_int(S), ref.cmp_int(S[np.arange(2 * n), np.concatenate([Xi[:, 2], Xi[:, 0]])])
    ptr, idx = FilterIndex(Xi).csr(Xi, L.EVAL_S_O, N_RING)
    fgt = np.array([(c[r, idx[ptr[r]:ptr[r + 1]]] > p[r]).sum() for r in range(2 * n)])
    feq = np.array([(c[r, idx[ptr[r]:ptr[r + 1]]] == p[r]).sum() for r in range(2 * n)])
    want = ranks_from_counts((c > p[:, None]).sum(1), (c == p[:, None]).sum(1), fgt, feq, n, "s,o", "worst")
    for prec in ("auto", 0):
        m.embedding_model_params["eval_precision"] = prec
        got = np.asarray(evaluate_performance(X, m, filter_triples=X))            # (model.get_ranks on an adapter)
        np.testing.assert_array_equal(got.reshape(want.shape), want)
        np.testing.assert_array_equal(m.get_ranks_idx(Xi, filter_idx=FilterIndex(Xi)), want)
    m.embedding_model_params["eval_precision"] = 2
    with pytest.raises(NotImplementedError, match="RotatE"):
        evaluate_performance(X, m, filter_triples=X)
    m.embedding_model_params["eval_precision"] = "auto"
    # predict, top-N, calibration, save / restore
    scores = m.predict(X)
    np.testing.assert_allclose(scores, ref.score_f64(E, R, Xi), rtol=1e-4, atol=1e-6)
    ents, sc = topn_completions(X[:5, :2], m, side="o", top_n=3)
    assert ents.shape == (5, 3) and np.all(np.diff(sc, axis=1) <= 0)
    neg = X.copy()
    neg[:, 2] = np.roll(X[:, 2], 7)
    m.calibrate(X, X_neg=neg)
    proba = m.predict_proba(X)
    assert proba.shape == (len(X),) and np.all((proba >= 0) & (proba <= 1))
    with pytest.raises(NotImplementedError, match="RotatE"):
        m.calibrate(X, positive_base_rate=0.5)
    path = str(tmp_path / "rotate.pkl")
    save_model(m, path)
    m2 = restore_model(path)
    assert type(m2).__name__ == "RotatE"
    np.testing.assert_array_equal(m2.predict(X), scores)
    np.testing.assert_array_equal(m2.predict_proba(X), proba)


def test_rank_through_link_regulariser_and_early_stopping():
    from emgraph_amd.evaluation import evaluate_performance
    X = _ring()
    m = _ring_model(epochs=30, loss="nll", optimizer="sgd", optimizer_params={"lr": 1e-12}, regularizer="LP",
                    regularizer_params={"p": 2, "lambda": 1e-5},
                    embedding_model_params={"non_linearity": "tanh", "rank_through_link": True})
    m.fit(X, early_stopping=True, early_stopping_params={"x_valid": X[:32], "criteria": "mrr", "burn_in": 0, "check_interval": 1,
                                                         "stop_interval": 2, "x_filter": X})
    assert m.is_fitted and m.early_stopping_epoch is not None and m.early_stopping_epoch <= 4   # (a rate too small to move a rank)
    assert not np.asarray(m.trained_model_params[1])[:, 8:].any()
    ranks = np.asarray(evaluate_performance(X[:16], m, filter_triples=X))
    assert ranks.shape == (16, 2) and ranks.min() >= 1


def test_entity_mode_discovery_reads_the_rows():
    from emgraph_amd.discovery import find_nearest_neighbours
    X = _ring()
    m = _ring_model(epochs=2)
    m.fit(X)
    nb, dist = find_nearest_neighbours(m, entities=["n00", "n01"], n_neighbors=3)
    assert np.asarray(nb).shape == (2, 3)
