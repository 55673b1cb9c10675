"""Relation negatives on the device (include/emgraph_hip.h: emg_relneg_forward / emg_relneg_backward; DESIGN.md A-28, 4.1 "Relation
negatives").  Draw j of positive i = (s, p, o) is (s, p', o), p' = idx + (idx >= p), idx = codes[j * B + i] in [0, n_rel - 1).

Bars: scores ``==`` on the bits to emg_eval_rel_scores_dense read at column p'; gradient rows ``==`` on the bits to the rows
emg_train_backward_ex(fused_loss = -1, eta = 0) writes for the pseudo-positives (s, p', o) (sums: float64 in ascending j, rounded
once); two runs byte-equal; one whole step against a float64 restatement within a bound derived from the roundings
(``_step_bound``); the public API runs, is deterministic, moves relation rows no positive of the batch names, survives save / restore
and early stopping."""
import itertools

import numpy as np
import pytest

from tests import _relneg_ref as ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32 = np.float32
EPS32 = 2.0 ** -24              # unit roundoff of float32
N_ENT = 40
SLICE = 32                      # csrc/emg_relneg.hip, kRnSlice: coordinates per LDS slice of the forward
WIDE = 2 * SLICE + 8            # two slices and a remainder (a multiple of 4: the 16-byte path crosses the boundaries too)
MODEL_IDS = {"TransE_L1": 0, "TransE_L2": 1, "DistMult": 2, "ComplEx": 3, "HolE": 4, "TransE_P": 5, "RotatE": 6, "SimplE": 8}
# (model, k_int): a complex model at k = 5 (scalar loads, a ragged tail), TransE at k = 8 (the 16-byte path), DistMult at 36 (16-byte
# path, a tail below a wave's width), and per chain kind a width of two LDS slices plus a remainder (WIDE coordinates; 71 / 75: the
# same through the scalar path) — every model id of emg_eval_rel_scores_dense
CASES = [("ComplEx", 10), ("HolE", 10), ("RotatE", 10), ("SimplE", 10), ("TransE_L1", 8), ("TransE_L2", 8), ("TransE_P", 8),
         ("DistMult", 36), ("DistMult", WIDE), ("DistMult", WIDE - 1), ("ComplEx", 2 * WIDE), ("HolE", 2 * WIDE), ("RotatE", 2 * WIDE),
         ("SimplE", 2 * WIDE), ("SimplE", 2 * (SLICE + 2)), ("TransE_L1", WIDE + 3), ("TransE_L2", WIDE), ("TransE_P", WIDE)]
BS, ETAS, N_RELS = (1, 67, 200), (1, 3, 20), (2, 3, 17)   # 67, 200: no multiples of a workgroup's run; eta * B no multiple of 64


def _scale(model):
    return {"HolE": 0.25, "TransE_P": 3.0, "SimplE": 0.5}.get(model, 1.0)


def _table(arr, pad):
    """device table with a row stride LARGER than its width (a multiple of 4 when ``pad`` is: rows stay 16-byte aligned)"""
    rows, k = arr.shape
    ld = ((k + 3) // 4) * 4 + pad
    buf = torch.zeros((rows, ld), dtype=torch.float32, device="cuda")
    view = buf[:, :k]
    view.copy_(torch.from_numpy(np.ascontiguousarray(arr, dtype=F32)))
    assert view.stride(0) > k
    return view


def _tables(model, ki, n_rel, seed):
    rs = np.random.RandomState(seed)
    if model == "RotatE":
        n = ki // 2
        E = (rs.randn(N_ENT, ki) * 0.7).astype(F32)
        R = np.concatenate([rs.uniform(-np.pi, np.pi, (n_rel, n)), np.zeros((n_rel, n))], 1).astype(F32)
        return E, R
    s = 0.8 if model.startswith("TransE") else 0.9
    return (rs.randn(N_ENT, ki) * s).astype(F32), (rs.randn(n_rel, ki) * s).astype(F32)


def _batch(B, eta, n_rel, seed):
    """positives with p = 0 and p = n_rel - 1 present (the two edges of the shift; B = 1: one of them, by the seed), and draws"""
    rs = np.random.RandomState(seed)
    pos = np.stack([rs.randint(0, N_ENT, B), rs.randint(0, n_rel, B), rs.randint(0, N_ENT, B)], 1).astype(np.int32)
    pos[0, 1] = 0 if (B > 1 or seed % 2 == 0) else n_rel - 1
    pos[-1, 1] = n_rel - 1 if B > 1 else pos[0, 1]
    idx = rs.randint(0, n_rel - 1, eta * B).astype(np.int32)
    return pos, idx


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _dense(model, Et, Rt, ki, post):
    """emg_eval_rel_scores_dense [B, n_rel] (RotatE: on the [cos | sin] image of the phase table, as the ranking calls it)"""
    from emgraph_amd import device as D
    rel = D.eval_rel_rotate_image(Rt, ki) if model == "RotatE" else Rt
    return D.eval_rel_scores_dense(MODEL_IDS[model], Et, rel, ki, _scale(model), post).cpu().numpy()


# ---- 1. scores to the bit ----
@pytest.mark.parametrize("model,ki", CASES)
def test_scores_have_the_bits_of_the_dense_relation_ranking_kernel(model, ki):
    from emgraph_amd import device as D
    D.require_gpu()
    mid, scale = MODEL_IDS[model], _scale(model)
    for n_rel in N_RELS:
        E, R = _tables(model, ki, n_rel, 11 + n_rel)
        Et, Rt = _table(E, 4), _table(R, 8)
        for B, eta in itertools.product(BS, ETAS):
            pos, idx = _batch(B, eta, n_rel, 100 * B + eta)
            post, codes = _dev(pos), _dev(idx)
            S = _dense(model, Et, Rt, ki, post)
            pp = ref.shift(idx, pos[:, 1])
            i = np.tile(np.arange(B), eta)
            assert (pp != pos[i, 1]).all()
            sp, sn = D.relneg_forward(mid, Et, Rt, ki, scale, post, eta, codes)
            got_n, got_p = sn.cpu().numpy(), sp.cpu().numpy()
            assert np.isfinite(got_n).all() and np.isfinite(got_p).all()
            assert np.array_equal(_bits(got_n), _bits(S[i, pp])), (model, ki, n_rel, B, eta)
            assert np.array_equal(_bits(got_p), _bits(S[np.arange(B), pos[:, 1]])), (model, ki, n_rel, B, eta)
            none, sn2 = D.relneg_forward(mid, Et, Rt, ki, scale, post, eta, codes, want_pos=False)   # the form beside entity sides
            assert none is None and np.array_equal(_bits(sn2.cpu().numpy()), _bits(got_n))


def test_scores_with_more_draws_than_a_workgroup_carries():
    """eta + 1 > 512 items per positive: the items are cut into slices for several workgroups, the last one scores the positive"""
    from emgraph_amd import device as D
    D.require_gpu()
    model, ki, n_rel, B, eta = "ComplEx", 10, 17, 3, 600
    E, R = _tables(model, ki, n_rel, 5)
    Et, Rt = _table(E, 4), _table(R, 4)
    pos, idx = _batch(B, eta, n_rel, 9)
    post = _dev(pos)
    S = _dense(model, Et, Rt, ki, post)
    sp, sn = D.relneg_forward(MODEL_IDS[model], Et, Rt, ki, 1.0, post, eta, _dev(idx))
    i = np.tile(np.arange(B), eta)
    assert np.array_equal(_bits(sn.cpu().numpy()), _bits(S[i, ref.shift(idx, pos[:, 1])]))
    assert np.array_equal(_bits(sp.cpu().numpy()), _bits(S[np.arange(B), pos[:, 1]]))


def test_an_index_outside_the_range_is_an_error_not_a_read():
    from emgraph_amd import _lib as L
    from emgraph_amd import device as D
    D.require_gpu()
    E, R = _tables("DistMult", 8, 3, 1)
    Et, Rt = _table(E, 4), _table(R, 4)
    pos, idx = _batch(5, 2, 3, 1)
    for bad in (2, -1, 1 << 30):                     # n_rel - 1 itself, a negative id, a keep bit's neighbourhood
        idx2 = idx.copy()
        idx2[3] = bad
        with pytest.raises(L.EmgError, match="outside"):
            D.relneg_forward(2, Et, Rt, 8, 1.0, _dev(pos), 2, _dev(idx2))
    sp, sn = D.relneg_forward(2, Et, Rt, 8, 1.0, _dev(pos), 2, _dev(idx))       # the flag does not stick
    assert np.isfinite(sn.cpu().numpy()).all()


# ---- 2. gradient rows to the bit ----
def _pseudo_rows(model, Et, Rt, ki, trip, g, raw):
    """the three gradient rows emg_train_backward_ex(fused_loss = -1, eta = 0) stores per triple of ``trip`` taken as positives under
    dL/dscore ``g``.  TransE-L2 takes its norm from the raw scores handed in (the same array the kernel under test gets)."""
    from emgraph_amd import device as D
    n = len(trip)
    ce = torch.zeros((2 * n, ki + 4), dtype=torch.float32, device="cuda")[:, :ki]
    cr = torch.zeros((n, ki + 4), dtype=torch.float32, device="cuda")[:, :ki]
    bw = dict(bw_scores_pos=raw) if model == "TransE_L2" else {}
    D.train_backward_ex(MODEL_IDS[model], Et, Rt, ki, _scale(model), _dev(trip.astype(np.int32)), 0, None, ce, cr, fused_loss=-1,
                        g_pos=g, **bw)
    ce, cr = ce.cpu().numpy(), cr.cpu().numpy()
    return ce[:n], ce[n:], cr


def _raw_scores(model, Et, Rt, ki, trip):
    """raw scores of the triples for the norm models.  TransE-p: emg_train_backward_ex recomputes its norm with the wave reduction
    of emg_train_forward, so the rows are comparable to the bit only under that norm: the raw scores are emg_train_forward's"""
    from emgraph_amd import device as D
    if model not in ("TransE_L2", "TransE_P"):
        return None
    return D.train_forward(MODEL_IDS[model], Et, Rt, ki, _scale(model), _dev(trip.astype(np.int32)), 0, None)[0]


def _backward(model, Et, Rt, ki, post, eta, codes, g_pos, g_neg, raw_pos, raw_neg, ldc_pad=4):
    from emgraph_amd import device as D
    B = post.shape[0]
    n_cr = (B if g_pos is not None else 0) + eta * B
    ldc = ((ki + 3) // 4) * 4 + ldc_pad
    ce = torch.full((2 * B, ldc), float("nan"), dtype=torch.float32, device="cuda")[:, :ki]
    cr = torch.full((n_cr, ldc), float("nan"), dtype=torch.float32, device="cuda")[:, :ki]
    de = torch.full((2 * B,), -7, dtype=torch.int32, device="cuda")
    dr = torch.full((n_cr,), -7, dtype=torch.int32, device="cuda")
    D.relneg_backward(MODEL_IDS[model], Et, Rt, ki, _scale(model), post, eta, codes, g_pos, g_neg, ce, cr, de, dr, raw_pos=raw_pos,
                      raw_neg=raw_neg)
    return ce.cpu().numpy(), cr.cpu().numpy(), de.cpu().numpy(), dr.cpu().numpy()


@pytest.mark.parametrize("model,ki", CASES)
@pytest.mark.parametrize("with_pos", [False, True])
def test_gradient_rows_have_the_bits_of_the_ordinary_backward(model, ki, with_pos):
    """eta = 1: the three rows per positive ARE the pseudo-positive's rows.  eta > 1: the s / o rows are the float64 sum of the
    per-draw rows in ascending j (after the positive's own term, when g_pos is given), rounded once; every relation row is one
    term; destinations (s | o), (p |) p'.  Two runs give the same bits."""
    from emgraph_amd import device as D
    D.require_gpu()
    combos = [(1, 1, 2), (67, 1, 3), (200, 1, 17), (67, 3, 17), (1, 20, 3), (200, 20, 2), (67, 20, 3)]
    for B, eta, n_rel in combos:
        E, R = _tables(model, ki, n_rel, 3 + n_rel)
        Et, Rt = _table(E, 4), _table(R, 8)
        pos, idx = _batch(B, eta, n_rel, 7 * B + eta)
        post, codes = _dev(pos), _dev(idx)
        rs = np.random.RandomState(B + eta)
        g_neg = _dev((rs.randn(eta * B) * 0.5).astype(F32))
        g_pos = _dev((rs.randn(B) * 0.5).astype(F32)) if with_pos else None
        neg = ref.negatives(pos, idx)
        raw_neg = _raw_scores(model, Et, Rt, ki, neg)
        raw_pos = _raw_scores(model, Et, Rt, ki, pos) if with_pos else None
        ce, cr, de, dr = _backward(model, Et, Rt, ki, post, eta, codes, g_pos, g_neg, raw_pos, raw_neg)
        assert np.isfinite(ce).all() and np.isfinite(cr).all(), (model, ki, B, eta, n_rel)
        P = B if with_pos else 0
        sum_s, sum_o = np.zeros((B, ki), np.float64), np.zeros((B, ki), np.float64)
        first = True
        if with_pos:
            rs_, ro_, rp_ = _pseudo_rows(model, Et, Rt, ki, pos, g_pos, raw_pos)
            sum_s, sum_o, first = rs_.astype(np.float64), ro_.astype(np.float64), False
            assert np.array_equal(_bits(cr[:B]), _bits(rp_)), (model, ki, B, eta, n_rel)
            assert np.array_equal(dr[:B], pos[:, 1])
        for j in range(eta):
            sl = slice(j * B, (j + 1) * B)
            rs_, ro_, rp_ = _pseudo_rows(model, Et, Rt, ki, neg[sl], g_neg[sl].contiguous(), raw_neg[sl].contiguous() if raw_neg is not None else None)
            if first:                                   # (the first term is taken as it is: the sign of a zero survives)
                sum_s, sum_o, first = rs_.astype(np.float64), ro_.astype(np.float64), False
            else:
                sum_s, sum_o = sum_s + rs_.astype(np.float64), sum_o + ro_.astype(np.float64)
            assert np.array_equal(_bits(cr[P + j * B:P + (j + 1) * B]), _bits(rp_)), (model, ki, B, eta, n_rel, j)
        assert np.array_equal(_bits(ce[:B]), _bits(sum_s.astype(F32))), (model, ki, B, eta, n_rel)
        assert np.array_equal(_bits(ce[B:]), _bits(sum_o.astype(F32))), (model, ki, B, eta, n_rel)
        assert np.array_equal(de, np.concatenate([pos[:, 0], pos[:, 2]]))
        assert np.array_equal(dr[P:], neg[:, 1])
        again = _backward(model, Et, Rt, ki, post, eta, codes, g_pos, g_neg, raw_pos, raw_neg)
        assert all(a.tobytes() == b.tobytes() for a, b in zip((ce, cr, de, dr), again))


def test_backward_through_the_scalar_stores():
    """rows of the contribution buffers that are not 16-byte aligned (ldc no multiple of 4): the scalar form writes the same bits"""
    from emgraph_amd import device as D
    D.require_gpu()
    model, ki, B, eta, n_rel = "DistMult", 36, 67, 3, 3
    E, R = _tables(model, ki, n_rel, 2)
    Et, Rt = _table(E, 4), _table(R, 4)
    pos, idx = _batch(B, eta, n_rel, 4)
    rs = np.random.RandomState(0)
    g_neg, g_pos = _dev(rs.randn(eta * B).astype(F32)), _dev(rs.randn(B).astype(F32))
    a = _backward(model, Et, Rt, ki, _dev(pos), eta, _dev(idx), g_pos, g_neg, None, None, ldc_pad=4)
    b = _backward(model, Et, Rt, ki, _dev(pos), eta, _dev(idx), g_pos, g_neg, None, None, ldc_pad=3)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_refusals_of_the_entry_points():
    from emgraph_amd import _lib as L
    from emgraph_amd import device as D
    D.require_gpu()
    E, R = _tables("TransE_P", 8, 3, 1)
    Et, Rt = _table(E, 4), _table(R, 4)
    pos, idx = _batch(5, 2, 3, 1)
    g = _dev(np.ones(10, F32))
    ce = torch.zeros((10, 8), dtype=torch.float32, device="cuda")
    cr = torch.zeros((10, 8), dtype=torch.float32, device="cuda")
    de, dr = torch.zeros(10, dtype=torch.int32, device="cuda"), torch.zeros(10, dtype=torch.int32, device="cuda")
    with pytest.raises(L.EmgError, match="raw"):                       # a norm model without its raw scores
        D.relneg_backward(5, Et, Rt, 8, 3.0, _dev(pos), 2, _dev(idx), None, g, ce, cr, de, dr)
    with pytest.raises(L.EmgError, match=r"code -3"):                  # EMG_ENOSUP: the maximum norm
        D.relneg_backward(5, Et, Rt, 8, float("inf"), _dev(pos), 2, _dev(idx), None, g, ce, cr, de, dr, raw_neg=g)
    with pytest.raises(L.EmgError, match="n_rel"):
        D.relneg_forward(2, Et, Rt[:1], 8, 1.0, _dev(pos), 2, _dev(idx))
    sp, sn = D.relneg_forward(5, Et, Rt, 8, float("inf"), _dev(pos), 2, _dev(idx))   # the forward has the maximum norm
    assert np.isfinite(sn.cpu().numpy()).all() and np.isfinite(sp.cpu().numpy()).all()


# ---- 3. one whole step ----
def _step_bound(lr32, G, absG, n_rows, w_new, opt, u=None):
    """Bound on |device - float64 restatement| per table element after ONE optimizer step from dL/dscore values both sides share.

    Gradient.  The model is DistMult: a term is g * (x * y), two correctly rounded multiplications -> relative error <= 2 eps (+ eps^2:
    2.1 eps is taken).  The relation side's s / o rows add their terms in double and round once: eps.  A destination's n terms (one
    per triple and role) are added in float32, inside the backward kernels and by the apply, in some order: at most n - 1 additions
    lie on the path of any term, each at most eps of a partial sum that is itself bounded by the sum of the terms' magnitudes absG.
    So  |dG| <= (2.1 + 1 + (n - 1)) eps absG.
    SGD.  w' = fl(w - fl(lr G)): lr |dG| + eps |lr G| + eps |w'|, and |lr G| <= lr absG.
    Adam, step 1 from zero state (emg_common.hpp::opt_update_elem, opt_ratio).  m = fl(1 - b1) g: 2 roundings; v = fl(1 - b2) g g: 3;
    lr_t m: 1; sqrt(v): half of v's relative error + the hardware square root's 1 ulp = 2 eps; + eps_hat: 1; the hardware
    reciprocal: 1 ulp = 2 eps; the product: 1 — 10.5 eps in all — and the relative error of g enters m once and sqrt(v) once:
    |du| <= |u| (10.5 eps + 2 |dG| / |G|), never more than 2 |u|_max = 2 lr (the step is lr sign(g) up to eps_hat); then the
    subtraction: eps |w'|.  eps = 2^-24."""
    dG = (2.1 + 1.0 + np.maximum(n_rows - 1, 0)[:, None]) * EPS32 * absG
    if opt == "sgd":
        return lr32 * dG + EPS32 * lr32 * absG + EPS32 * np.abs(w_new)
    rel = 10.5 * EPS32 + 2.0 * dG / np.maximum(np.abs(G), 1e-300)
    return np.minimum(np.abs(u) * rel, 2.0 * lr32) + EPS32 * np.abs(w_new)


@pytest.mark.parametrize("sides", [["p"], ["s", "p"]])
@pytest.mark.parametrize("opt,link", [("sgd", "linear"), ("sgd", "tanh"), ("adam", "linear")])
def test_one_step_against_a_float64_restatement(sides, opt, link):
    """Trainer(corrupt_sides=sides), one step: the codes are the restated draws (entity sides as ever, then 'p' under counter0 +
    sd_p), and the tables move as the update rule says for the float64 gradient of sum(g * score) with the device's OWN g_pos / g_neg
    (read back after emg_loss and the link's chain rule).  n_rel = 3: many draws land on one relation row."""
    from emgraph_amd import _lib as L
    from emgraph_amd import device as D
    from emgraph_amd.training import Trainer
    from tests import _negsample_ref as ns
    D.require_gpu()
    ki, n_rel, B, eta, seed, lr, epoch, batch, bc = 12, 3, 67, 3, 7, 0.05, 2, 3, 4
    rs = np.random.RandomState(17)
    E0, R0 = (rs.randn(N_ENT, ki) * 0.6).astype(F32), (rs.randn(n_rel, ki) * 0.6).astype(F32)
    X = np.stack([rs.randint(0, N_ENT, B), rs.randint(0, n_rel, B), rs.randint(0, N_ENT, B)], 1).astype(np.int32)
    tr = Trainer(L.DISTMULT, ki, 1.0, E0, R0, eta, loss="nll", optimizer=opt, optimizer_params={"lr": lr}, corrupt_sides=sides,
                 batches_count=bc, seed=seed, link=link)
    tr.set_training_set(X, B)
    assert tr.plan is None and tr.relneg and not tr.fused
    tr.step(0, B, epoch=epoch, batch=batch)
    torch.cuda.synchronize()
    E1, R1 = tr.tables_numpy()
    n_sides, n_e = len(sides), len(sides) - 1
    et = eta * n_sides
    codes = tr.slots[0]["codes"][:et * B].cpu().numpy()
    g_pos, g_neg = tr.g_pos[:B].cpu().numpy().astype(np.float64), tr.g_neg[:et * B].cpu().numpy().astype(np.float64)
    assert np.isfinite(g_pos).all() and np.isfinite(g_neg).all() and np.abs(g_neg).max() > 0
    # the draws: side sd under counter0 + sd, the relation side last over n_rel - 1 choices
    counter0 = ((epoch - 1) * bc + (batch - 1)) * n_sides
    trips, gs = [X.astype(np.int64)], [g_pos]
    for sd, side in enumerate(sides[:n_e]):
        part = ns.sample_side(X, eta, side, seed, counter0 + sd, N_ENT)
        assert np.array_equal(codes[sd * eta * B:(sd + 1) * eta * B], part["codes"])
        trips.append(part["neg"].astype(np.int64))
    idx = ref.draw_idx(B, eta, n_rel, seed, counter0 + n_e)
    assert np.array_equal(codes[n_e * eta * B:], idx.astype(np.int32))
    trips.append(ref.negatives(X, idx))
    trip = np.concatenate(trips, 0)
    g = np.concatenate([g_pos, g_neg])
    dE, dR, absE, absR = ref.dense_grads(ref.DISTMULT, E0, R0, trip, g, 1.0)
    # terms per destination: one per (triple, role) — every path of additions to a row's sum is at most that long
    cnt_e, cnt_r = np.zeros(N_ENT), np.zeros(n_rel)
    np.add.at(cnt_e, trip[:, 0], 1)
    np.add.at(cnt_e, trip[:, 2], 1)
    np.add.at(cnt_r, trip[:, 1], 1)
    lr32 = float(F32(lr))
    for W0, W1, G, absG, cnt in ((E0, E1, dE, absE, cnt_e), (R0, R1, dR, absR, cnt_r)):
        W0 = W0.astype(np.float64)
        if opt == "sgd":
            want, u = W0 - lr32 * G, None
        else:
            b1, b2, eps_hat = float(F32(0.9)), float(F32(0.999)), float(F32(1e-7))
            lr_t = float(F32(lr * np.sqrt(1.0 - 0.999) / (1.0 - 0.9)))
            m, v = (1.0 - b1) * G, (1.0 - b2) * G * G
            u = lr_t * m / (np.sqrt(v) + eps_hat)
            want = W0 - u
        bound = _step_bound(lr32, G, absG, cnt, want, opt, u)
        err = np.abs(W1.astype(np.float64) - want)
        print("relneg step", sides, opt, link, "max err / bound", float((err / np.maximum(bound, 1e-300)).max()), "max err", float(err.max()))
        assert (err <= bound).all(), (sides, opt, link, float((err / np.maximum(bound, 1e-300)).max()))
        untouched = cnt == 0
        assert np.array_equal(W1[untouched], W0.astype(F32)[untouched])
    assert np.abs(R1 - R0).max() > 0 and np.isfinite(tr.read_loss())


# ---- 4. public API ----
def _toy_graph():
    """300 triples over 40 entities and 4 relations, sorted so that rows [0, 150) name relations 0 and 1 only"""
    rs = np.random.RandomState(21)
    n_ent, n_rel, n = 40, 4, 300
    X = np.stack([rs.randint(0, n_ent, n), np.r_[rs.randint(0, 2, n // 2), rs.randint(2, 4, n // 2)], rs.randint(0, n_ent, n)], 1)
    X[:n_ent, 0] = np.arange(n_ent)          # every entity and relation occurs: labels == ids after mapping
    X[:2, 1], X[n // 2:n // 2 + 2, 1] = [0, 1], [2, 3]
    return X.astype(np.int64), n_ent, n_rel


def _fit(X, n_ent, n_rel, sides, **kw):
    from emgraph_amd.models import ComplEx
    k = 8
    rs = np.random.RandomState(5)
    ent0, rel0 = (rs.randn(n_ent, 2 * k) * 0.4).astype(F32), (rs.randn(n_rel, 2 * k) * 0.4).astype(F32)
    m = ComplEx(k=k, eta=3, epochs=kw.pop("epochs", 2), batches_count=2, seed=3, loss="nll", optimizer="adam", optimizer_params={"lr": 0.01},
                embedding_model_params={"corrupt_sides": sides}, initializer="constant",
                initializer_params={"entity": ent0, "relation": rel0})
    m.fit(X, **kw)
    return m, ent0, rel0


def test_fit_with_relation_negatives(tmp_path):
    from emgraph_amd import device as D
    from emgraph_amd.utils import restore_model, save_model
    D.require_gpu()
    X, n_ent, n_rel = _toy_graph()
    m, ent0, rel0 = _fit(X, n_ent, n_rel, ["s,o", "p"])
    assert np.all(np.isfinite(m.epoch_losses)) and np.isfinite(m.trained_model_params[0]).all() and np.isfinite(m.trained_model_params[1]).all()
    assert m._trainer.relneg and m._trainer.n_sides == 2
    assert m.negative_sampling_stats == {"rows": 2 * 300 * 3 * 2, "redrawn": 0, "known_left": 0}   # not extended: rows of both sides
    # deterministic under the seed
    m2, _, _ = _fit(X, n_ent, n_rel, ["p", "s,o"])                       # (the same list after canonicalisation)
    assert m2.trained_model_params[0].tobytes() == m.trained_model_params[0].tobytes()
    assert m2.trained_model_params[1].tobytes() == m.trained_model_params[1].tobytes() and m2.epoch_losses == m.epoch_losses
    # the entity-only fit is another run
    m3, _, _ = _fit(X, n_ent, n_rel, ["s,o"])
    assert not np.array_equal(m3.trained_model_params[1], m.trained_model_params[1])
    # the key travels through save / restore; prediction does not know about it
    path = str(tmp_path / "relneg.pkl")
    save_model(m, path)
    r = restore_model(path)
    assert r.embedding_model_params["corrupt_sides"] == ["s,o", "p"]
    np.testing.assert_array_equal(r.predict(X[:20]), m.predict(X[:20]))


@pytest.mark.parametrize("sides", [["p"], ["s,o", "p"]])
def test_a_step_moves_relation_rows_no_positive_of_the_batch_names(sides):
    """fit() itself visits every relation of X in some batch, so the property is shown on ONE step of a fitted model's trainer
    (plain SGD: a row without a gradient row stays as it is, bit for bit) over rows [0, 150), whose positives name relations 0 and 1
    only: relations 2 and 3 move — only relation negatives can do that.  With ['s,o'] they stay."""
    from emgraph_amd import device as D
    from emgraph_amd.models import ComplEx
    D.require_gpu()
    X, n_ent, n_rel = _toy_graph()
    assert set(X[:150, 1]) == {0, 1}

    def one_more_step(sd):
        m = ComplEx(k=8, eta=3, epochs=1, batches_count=2, seed=3, loss="nll", optimizer="sgd", optimizer_params={"lr": 0.05},
                    embedding_model_params={"corrupt_sides": sd})
        m.fit(X)
        tr = m._trainer
        before = tr.tables_numpy()[1].copy()
        tr.step(0, 150, epoch=2, batch=1)
        return before, tr.tables_numpy()[1]

    before, after = one_more_step(sides)
    assert (np.abs(after[2:] - before[2:]).max(axis=1) > 0).all() and (np.abs(after[:2] - before[:2]).max(axis=1) > 0).all()
    before, after = one_more_step(["s,o"])
    assert np.array_equal(after[2:], before[2:]) and (np.abs(after[:2] - before[:2]).max(axis=1) > 0).all()


def test_early_stopping_runs_with_relation_negatives():
    from emgraph_amd import device as D
    D.require_gpu()
    X, n_ent, n_rel = _toy_graph()
    m, _, _ = _fit(X, n_ent, n_rel, ["s,o", "p"], epochs=4, early_stopping=True,
                   early_stopping_params={"x_valid": X[::10], "criteria": "mrr", "burn_in": 1, "check_interval": 1, "stop_interval": 2,
                                          "x_filter": X})
    assert m.is_fitted and 1 <= len(m.epoch_losses) <= 4 and np.all(np.isfinite(m.epoch_losses))
