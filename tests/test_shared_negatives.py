"""Shared negatives on the device (include/emgraph_hip.h: emg_shared_forward / emg_shared_backward; DESIGN.md A-26, 4.1 "Shared
negatives").  Everything rests on one identity: the shared step is the ordinary step with
``codes[m * B + i] = chunk_codes[m * G + i // C]`` (tests/_shared_ref.py) — so the ordinary step, driven with the expanded codes, is
the reference.

Bars: scores ``==`` on the bits to emg_eval_build_queries + emg_eval_scores_dense; gradient tables (rows added by destination in
float64) at most 4x the ordinary backward's max-norm error against a float64 restatement; the step against the ordinary step within
tests/test_api.py's fit() bar (tables rtol 2e-3 / atol 2e-5, losses rtol 2e-4 / atol 1e-6); two runs byte-equal."""
import numpy as np
import pytest

from tests import _shared_ref as ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32 = np.float32
N_ENT, N_REL = 50, 4            # few entities: a chunk's draws repeat and hit its own positives' entities
B, C, ETA = 70, 16, 3           # 5 chunks, the last one holds 6 rows
GRID = 1.0 / 512                # TransE tables live on a grid: entity entries even, relation entries odd multiples of GRID
MODELS = ("TransE_L1", "TransE_L2", "DistMult", "ComplEx", "HolE", "TransE_P", "RotatE")
PAIRED = ("ComplEx", "HolE", "RotatE")
SIDES = (("s,o",), ("s",), ("s", "o"))
TABLE_TOL = dict(rtol=2e-3, atol=2e-5)      # tests/test_api.py: fit() against the oracle
LOSS_TOL = dict(rtol=2e-4, atol=1e-6)


def _away_from_zero(model, ki, E, R, trip):
    """smallest |e_s + r_p - e_o| entry (TransE) / smallest modulus |s o r - o| (RotatE) over the triples; inf for the other models"""
    if model.startswith("TransE"):
        return float(np.abs(E[trip[:, 0]].astype(np.float64) + R[trip[:, 1]] - E[trip[:, 2]]).min())
    if model == "RotatE":
        n = ki // 2
        a, th, b = E[trip[:, 0]].astype(np.float64), R[trip[:, 1], :n].astype(np.float64), E[trip[:, 2]].astype(np.float64)
        return float(np.abs((a[:, :n] + 1j * a[:, n:]) * np.exp(1j * th) - (b[:, :n] + 1j * b[:, n:])).min())
    return np.inf


def _mid(model):
    return MODELS.index(model)


def _scale(model):
    return {"HolE": 0.25, "TransE_P": 3.0}.get(model, 1.0)


def _tables(model, ki, seed, n_ent=N_ENT, n_rel=N_REL, grid=True):
    """scores of order one at any width.  TransE (``grid``): every difference e_s + r_p - e_o is an ODD multiple of GRID (|d| >=
    1.9e-3 in every column of every triple: no subgradient choice at |d| = 0); RotatE: phases in [-pi, pi), zeros in the unused half"""
    rs = np.random.RandomState(seed)
    if model.startswith("TransE") and not grid:
        return (rs.randn(n_ent, ki) * (1.5 / ki)).astype(F32), (rs.randn(n_rel, ki) * (1.5 / ki)).astype(F32)
    if model.startswith("TransE"):
        span = 6 if ki > 64 else 60
        E = (2 * rs.randint(-span, span + 1, (n_ent, ki)) * GRID).astype(F32)
        R = ((2 * rs.randint(-span, span + 1, (n_rel, ki)) + 1) * GRID).astype(F32)
        return E, R
    if model == "RotatE":
        n = ki // 2
        E = (rs.randn(n_ent, ki) * (1.0 if grid and n > 64 else 1.0 / n)).astype(F32)   # (wide rows: moduli of order one, none near 0)
        R = np.concatenate([rs.uniform(-np.pi, np.pi, (n_rel, n)), np.zeros((n_rel, n))], 1).astype(F32)
        return E, R
    sigma = (2.0 * ki) ** (-1 / 6) if model in PAIRED else float(ki) ** (-1 / 6)
    return (rs.randn(n_ent, ki) * sigma).astype(F32), (rs.randn(n_rel, ki) * sigma).astype(F32)


def _positives(seed, n=B):
    rs = np.random.RandomState(1000 + seed)
    return np.stack([rs.randint(0, N_ENT, n), rs.randint(0, N_REL, n), rs.randint(0, N_ENT, n)], 1).astype(np.int32)


def _side_ids(sides):
    from emgraph_amd import _lib as L
    return [L.SIDE_IDS[s] for s in sides]


def _chunk_codes(n_rows, C_, sides, seed, counter0, n_choices=N_ENT, entities_list=None, eta=ETA):
    """what Trainer(shared_negatives=C_) draws for a batch: per side, emg_corrupt_codes with B := G under that side's counter"""
    from emgraph_amd import device as D
    G = ref.n_chunks(n_rows, C_)
    return torch.cat([D.corrupt_codes(G, eta, sd, n_choices, "cuda", entities_list=entities_list, seed=seed, counter=counter0 + i)
                      for i, sd in enumerate(_side_ids(sides))])


def _dev_tables(E, R, ki):
    from emgraph_amd.training import alloc_table
    dev = torch.device("cuda")
    return alloc_table(E.shape[0], ki, dev, init=E), alloc_table(R.shape[0], ki, dev, init=R)


CASES = [(m, ki) for m in MODELS for ki in ((10 if m in PAIRED else 5), 8, 400)]


# ---- 1. scores to the bit ----
@pytest.mark.parametrize("model,ki", CASES)
def test_scores_have_the_bits_of_the_dense_ranking_kernel(model, ki):
    from emgraph_amd import _lib as L
    from emgraph_amd import device as D
    D.require_gpu()
    E, R = _tables(model, ki, 11, grid=False)      # (sums of grid values would be exact in any order)
    Et, Rt = _dev_tables(E, R, ki)
    pos = _positives(1)
    post = torch.from_numpy(pos).cuda()
    mid, scale = _mid(model), _scale(model)
    Q, _ = D.eval_build_queries(mid, Et, Rt, ki, scale, post, L.EVAL_S_O)     # rows [0, B) object side, [B, 2B) subject side
    S = D.eval_scores_dense(mid, Q, Et, ki, scale).cpu().numpy()              # [2B, N_ENT]
    hit_own = 0
    for sides in SIDES:
        et = ETA * len(sides)
        cc = _chunk_codes(B, C, sides, seed=5, counter0=2)
        sp, sn = D.shared_forward(mid, Et, Rt, ki, scale, post, C, et, cc)
        codes = ref.expand_codes(cc.cpu().numpy(), B, C, et)
        assert np.array_equal(codes, D.expand_shared_codes(cc, B, C, et).cpu().numpy())
        repl, keep = ref.split_codes(codes)
        i = np.tile(np.arange(B), et)
        want = np.where(keep == 1, S[i, repl], S[B + i, repl])
        got_n, got_p = sn.cpu().numpy(), sp.cpu().numpy()
        assert np.array_equal(got_n.view(np.uint32), want.astype(F32).view(np.uint32)), (model, ki, sides)
        assert np.array_equal(got_p.view(np.uint32), S[np.arange(B), pos[:, 2]].view(np.uint32)), (model, ki, sides)
        assert np.isfinite(got_n).all() and np.isfinite(got_p).all()
        hit_own += int(((repl == pos[i, 0]) | (repl == pos[i, 2])).sum())
        if "s,o" in sides:
            assert 0 < keep.sum() < keep.size                                  # both kinds of draw in one launch
    assert hit_own > 0, "no draw hit an entity of its own chunk's positives: the case the small table is there for"


@pytest.mark.parametrize("model,ki,C_,n,eta", [("ComplEx", 8, 256, 600, 5), ("TransE_L1", 5, 128, 300, 9), ("RotatE", 10, 256, 300, 5),
                                               ("HolE", 400, 256, 257, 5), ("DistMult", 8, 1, 700, 3)])
def test_scores_in_the_other_launch_shapes(model, ki, C_, n, eta):
    """more draws per chunk than a workgroup's threads carry pairs for (C_ * eta_total > 2048): the chunk's draws are cut into slices
    for several workgroups, slice 0 scores the positives; chunks of more than ~190 rows: column blocks of 16; chunks of one row"""
    from emgraph_amd import _lib as L
    from emgraph_amd import device as D
    D.require_gpu()
    E, R = _tables(model, ki, 13, grid=False)
    Et, Rt = _dev_tables(E, R, ki)
    pos = _positives(4, n)
    post = torch.from_numpy(pos).cuda()
    mid, scale, sides = _mid(model), _scale(model), ("s", "o")
    et = eta * len(sides)
    assert C_ == 1 or C_ * et > 2048
    Q, _ = D.eval_build_queries(mid, Et, Rt, ki, scale, post, L.EVAL_S_O)
    S = D.eval_scores_dense(mid, Q, Et, ki, scale).cpu().numpy()
    cc = _chunk_codes(n, C_, sides, seed=8, counter0=0, eta=eta)
    sp, sn = D.shared_forward(mid, Et, Rt, ki, scale, post, C_, et, cc)
    repl, keep = ref.split_codes(D.expand_shared_codes(cc, n, C_, et).cpu().numpy())
    i = np.tile(np.arange(n), et)
    want = np.where(keep == 1, S[i, repl], S[n + i, repl]).astype(F32)
    assert np.array_equal(sn.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(sp.cpu().numpy().view(np.uint32), S[np.arange(n), pos[:, 2]].view(np.uint32))


# ---- 2. gradient rows ----
@pytest.mark.parametrize("model,ki", CASES)
def test_gradient_rows_against_the_ordinary_backward(model, ki, capsys):
    _check_gradient_rows(model, ki, capsys, B, C)


@pytest.mark.parametrize("model,ki", [("ComplEx", 8), ("TransE_L2", 5), ("RotatE", 400), ("DistMult", 400)])
def test_gradient_rows_of_the_largest_chunks(model, ki, capsys):
    """C = 256: the backward stages 768 rows and the chunk's draws in column blocks of 16; the last chunk holds 44 rows"""
    _check_gradient_rows(model, ki, capsys, 300, 256)


def _check_gradient_rows(model, ki, capsys, B, C):
    from emgraph_amd import device as D
    D.require_gpu()
    pos = _positives(2, B)
    post = torch.from_numpy(pos).cuda()
    mid, scale = _mid(model), _scale(model)
    dev = torch.device("cuda")
    rs = np.random.RandomState(7)
    all_codes = [D.expand_shared_codes(_chunk_codes(B, C, sides, seed=6, counter0=4), B, C, ETA * len(sides)).cpu().numpy() for sides in SIDES]
    all_trip = np.concatenate([pos.astype(np.int64)] + [ref.negatives(pos, c, ETA * len(sd)) for c, sd in zip(all_codes, SIDES)], 0)
    for data_seed in range(12, 32):     # the first tables that meet the precondition below for every triple of every side list
        E, R = _tables(model, ki, data_seed)
        if _away_from_zero(model, ki, E, R, all_trip) >= 1e-3:
            break
    Et, Rt = _dev_tables(E, R, ki)
    ld = Et.stride(0)
    for sides in SIDES:
        et = ETA * len(sides)
        G = ref.n_chunks(B, C)
        cc = _chunk_codes(B, C, sides, seed=6, counter0=4)
        codes_t = D.expand_shared_codes(cc, B, C, et)
        codes = codes_t.cpu().numpy()
        # the precondition: no |difference| (TransE) and no modulus (RotatE) below 1e-3 — no subgradient choice is compared
        trip = np.concatenate([pos.astype(np.int64), ref.negatives(pos, codes, et)], 0)
        assert _away_from_zero(model, ki, E, R, trip) >= 1e-3
        g_pos = rs.randn(B).astype(F32)
        g_neg = rs.randn(et * B).astype(F32)
        gp_t, gn_t = torch.from_numpy(g_pos).cuda(), torch.from_numpy(g_neg).cuda()
        sp, sn = D.shared_forward(mid, Et, Rt, ki, scale, post, C, et, cc)
        # new: 2B + et * G entity rows
        n_ce = 2 * B + et * G
        ce = torch.full((n_ce, ld), float("nan"), dtype=torch.float32, device=dev)[:, :ki]
        cr = torch.full((B, ld), float("nan"), dtype=torch.float32, device=dev)[:, :ki]
        de = torch.full((n_ce,), -1, dtype=torch.int32, device=dev)
        dr = torch.full((B,), -1, dtype=torch.int32, device=dev)
        D.shared_backward(mid, Et, Rt, ki, scale, post, C, et, cc, gp_t, gn_t, ce, cr, de, dr, raw_pos=sp, raw_neg=sn)
        de_h, dr_h = de.cpu().numpy(), dr.cpu().numpy()
        repl_c, _ = ref.split_codes(cc.cpu().numpy())
        assert np.array_equal(de_h, np.concatenate([pos[:, 0], pos[:, 2], repl_c])) and np.array_equal(dr_h, pos[:, 1])
        new_E = ref.scatter_rows(ce.cpu().numpy(), de_h, N_ENT)
        new_R = ref.scatter_rows(cr.cpu().numpy(), dr_h, N_REL)
        assert np.isfinite(new_E).all() and np.isfinite(new_R).all()           # every row and column was written
        # the ordinary backward on the expanded codes: (2 + et) B entity rows
        n_pe = (2 + et) * B
        pe = torch.zeros((n_pe, ld), dtype=torch.float32, device=dev)[:, :ki]
        pr = torch.zeros((B, ld), dtype=torch.float32, device=dev)[:, :ki]
        pde = torch.empty(n_pe, dtype=torch.int32, device=dev)
        pdr = torch.empty(B, dtype=torch.int32, device=dev)
        D.build_dest(post, et, codes_t, pde, pdr)
        D.train_backward_ex(mid, Et, Rt, ki, scale, post, et, codes_t, pe, pr, fused_loss=-1, g_pos=gp_t, g_neg=gn_t)
        par_E = ref.scatter_rows(pe.cpu().numpy(), pde.cpu().numpy(), N_ENT)
        par_R = ref.scatter_rows(pr.cpu().numpy(), pdr.cpu().numpy(), N_REL)
        want_E, want_R = ref.dense_grads(mid, E, R, pos, codes, et, g_pos, g_neg, scale)
        for name, new, par, want in (("ent", new_E, par_E, want_E), ("rel", new_R, par_R, want_R)):
            e_new, e_par = np.abs(new - want).max(), np.abs(par - want).max()
            with capsys.disabled():
                print("\nshared-negatives gradient error %-9s k_int %3d %-9s %s: new %.3e  ordinary %.3e  ratio %.2f  (max |g| %.2e)"
                      % (model, ki, ",".join(sides), name, e_new, e_par, e_new / max(e_par, 1e-300), np.abs(want).max()))
            assert e_par <= 1e-4 * max(1.0, np.abs(want).max()), "the reference restatement and the ordinary backward disagree"
            assert e_new <= 4.0 * e_par, (model, ki, sides, name, e_new, e_par)


# ---- 3 - 5. the step against the ordinary step ----
N_STEPS = 5
STEP_MODELS = {"TransE_L1": 8, "ComplEx": 16, "RotatE": 16}      # k_int


def _trainer(model, ki, E, R, sides, loss, opt, seed, extra=None, **kw):
    from emgraph_amd.training import Trainer
    lr = {"sgd": 0.05, "momentum": 0.02, "adagrad": 0.05, "adam": 0.01}[opt]
    args = dict(loss=loss, loss_params={"margin": 1.0 if loss != "self_adversarial" else 3.0, "alpha": 0.5}, optimizer=opt,
                optimizer_params={"lr": lr}, corrupt_sides=sides, batches_count=N_STEPS, seed=seed)
    args.update(extra or {})
    args.update(kw)
    return Trainer(_mid(model), ki, _scale(model), E, R, ETA, **args)


def _pool(pool):
    """(n_choices, entities_list) of a negative pool: None = all entities | int = the first ids | list = those ids"""
    if pool is None:
        return N_ENT, None
    if isinstance(pool, int):
        return pool, None
    return len(pool), torch.tensor(pool, dtype=torch.int32, device="cuda")


def _run_shared(model, ki, E, R, X, sides, loss, opt, seed, C_=C, extra=None, edge_w=None, pool=None):
    """N_STEPS shared steps; returns (tables, loss, min distance of a hinge argument from 0 over all steps, draws counted)"""
    tr = _trainer(model, ki, E, R, sides, loss, opt, seed, extra, shared_negatives=C_)
    tr.set_training_set(X, B, edge_w=edge_w)
    et = ETA * len(sides)
    away = np.inf
    n_choices, elist = _pool(pool)
    for b in range(1, N_STEPS + 1):
        nb = min(B, len(X) - (b - 1) * B)           # (the last batch may be short)
        tr.step((b - 1) * B, nb, epoch=1, batch=b, n_choices=n_choices, entities_list=elist)
        if loss in ("pairwise", "absolute_margin"):
            s = tr.scores_all[:nb * (1 + et)].cpu().numpy().astype(np.float64)    # the (effective) scores the loss saw
            sp, sn = s[:nb], s[nb:].reshape(et, nb)
            v = (tr.margin - sp[None, :] + sn) if loss == "pairwise" else (tr.margin + sn)
            away = min(away, float(np.abs(v).min()))
    Eo, Ro = tr.tables_numpy()
    return Eo, Ro, tr.read_loss(), away, tr.negative_sampling_stats()["rows"]


def _run_ordinary(model, ki, E, R, X, sides, loss, opt, seed, C_=C, extra=None, edge_w=None, inject=True, pool=None):
    """the parent's host-visible step, driven with the expansion of the draws the shared step makes (``inject``) or left alone"""
    from emgraph_amd import device as D
    tr = _trainer(model, ki, E, R, sides, loss, opt, seed, extra, fused=False, inplace=False, pipeline=False)
    tr.set_training_set(X, B, edge_w=edge_w)
    et = ETA * len(sides)
    for b in range(1, N_STEPS + 1):
        kw = {}
        nb = min(B, len(X) - (b - 1) * B)
        if inject:
            n_choices, elist = _pool(pool)      # (the codes hold the pool's entity ids: injected as they are)
            cc = _chunk_codes(nb, C_, sides, seed=seed, counter0=(b - 1) * len(sides), n_choices=n_choices, entities_list=elist)
            if pool is not None:
                ids = set(range(pool)) if isinstance(pool, int) else set(pool)
                assert set((cc & 0x7FFFFFFF).cpu().numpy().tolist()) <= ids
            codes = D.expand_shared_codes(cc, nb, C_, et)
            kw = dict(inj_repl=(codes & 0x7FFFFFFF).contiguous(), inj_mask=(codes < 0).to(torch.int32).contiguous())
        tr.step((b - 1) * B, nb, epoch=1, batch=b, **kw)
    Eo, Ro = tr.tables_numpy()
    return Eo, Ro, tr.read_loss()


def _compare_steps(model, sides, loss, opt, extra=None, focuse=False, C_=C, inject=True, pool=None, short=0):
    from emgraph_amd import device as D
    D.require_gpu()
    ki = STEP_MODELS[model]
    X = _positives(3, N_STEPS * B - short)
    hinged = loss in ("pairwise", "absolute_margin")
    for data_seed in range(20):         # hinged losses: the first tables none of whose pairs comes within 1e-3 of the kink
        E, R = _tables(model, ki, 40 + data_seed)
        edge_w = np.random.RandomState(9).uniform(0, 1, len(X)).astype(F32) if focuse else None
        Es, Rs, ls, away, rows = _run_shared(model, ki, E, R, X, sides, loss, opt, 17, C_, extra, edge_w, pool)
        if not hinged or away >= 1e-3:
            break
    assert not hinged or away >= 1e-3, "precondition: no tables found that keep every pair 1e-3 away from the hinge"
    assert rows == ((N_STEPS - 1) * ref.n_chunks(B, C_) + ref.n_chunks(B - short, C_)) * ETA * len(sides)
    Eo, Ro, lo = _run_ordinary(model, ki, E, R, X, sides, loss, opt, 17, C_, extra, edge_w, inject, pool)
    what = str((model, sides, loss, opt, extra, focuse, C_))
    assert not np.allclose(Es, E, atol=1e-6), "the step did not move the tables"
    np.testing.assert_allclose(Es, Eo, err_msg=what, **TABLE_TOL)
    np.testing.assert_allclose(Rs, Ro, err_msg=what, **TABLE_TOL)
    np.testing.assert_allclose(ls, lo, err_msg=what, **LOSS_TOL)
    assert np.isfinite(ls)


@pytest.mark.parametrize("opt", ["sgd", "adam"])
@pytest.mark.parametrize("loss", ["pairwise", "nll", "absolute_margin", "self_adversarial", "multiclass_nll"])
@pytest.mark.parametrize("model", list(STEP_MODELS))
def test_step_equals_the_ordinary_step_on_the_expanded_codes(model, loss, opt):
    sides = {"TransE_L1": ("s,o",), "ComplEx": ("s", "o"), "RotatE": ("s,o",)}[model]
    _compare_steps(model, sides, loss, opt)


@pytest.mark.parametrize("model,opt,extra", [
    ("TransE_L1", "adagrad", None),
    ("ComplEx", "momentum", None),
    ("RotatE", "sgd", dict(regularizer="LP", regularizer_params={"p": 2, "lambda": 1e-3})),
    ("ComplEx", "adam", dict(regularizer="LP", regularizer_params={"p": 2, "lambda": 1e-3})),
    ("TransE_L1", "sgd", dict(normalize_ent_emb=True)),
])
def test_step_with_the_other_optimizers_and_the_folded_regulariser(model, opt, extra):
    _compare_steps(model, ("s,o",), "nll", opt, extra=extra)


def test_step_with_a_tanh_link_and_focuse_weights():
    _compare_steps("ComplEx", ("s,o",), "nll", "adam", extra=dict(link="tanh", focuse_params={"stop_epoch": 0, "structural_wt": 0.3}),
                   focuse=True)
    _compare_steps("TransE_L1", ("s",), "self_adversarial", "sgd", extra=dict(link="tanh"))


def test_step_with_a_short_last_batch():
    """the last batch holds 45 rows (chunks of 16, 16, 13) where the scratch was laid out for 70"""
    _compare_steps("ComplEx", ("s", "o"), "self_adversarial", "adam", short=25)
    _compare_steps("RotatE", ("s,o",), "nll", "sgd", short=25, C_=1, inject=False)


# ---- 4. C = 1 ----
@pytest.mark.parametrize("model,sides", [("ComplEx", ("s,o",)), ("TransE_L1", ("s", "o")), ("RotatE", ("o",))])
def test_chunks_of_one_are_the_ordinary_step_with_its_own_draws(model, sides):
    """no injection: this pins the draws and their counters"""
    _compare_steps(model, sides, "nll", "adam", C_=1, inject=False)


# ---- 5. determinism ----
def test_two_runs_give_the_same_bytes():
    from emgraph_amd import device as D
    D.require_gpu()
    E, R = _tables("ComplEx", 16, 40)
    X = _positives(3, N_STEPS * B)
    a = _run_shared("ComplEx", 16, E, R, X, ("s", "o"), "nll", "adam", 17)
    b = _run_shared("ComplEx", 16, E, R, X, ("s", "o"), "nll", "adam", 17)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]


# ---- 6. public API ----
def _toy_graph():
    rs = np.random.RandomState(21)
    n_ent, n_rel, n = 40, 3, 300
    X = np.stack([rs.randint(0, n_ent, n), rs.randint(0, n_rel, n), rs.randint(0, n_ent, n)], 1)
    X[:n_ent, 0] = np.arange(n_ent)          # every entity and relation occurs: labels == ids after mapping
    X[:n_rel, 1] = np.arange(n_rel)
    return X.astype(np.int64), n_ent, n_rel


def test_fit_with_the_key_equals_the_trainer_level_loop(tmp_path):
    from emgraph_amd import device as D
    from emgraph_amd.models import ComplEx
    from emgraph_amd.training import Trainer
    from emgraph_amd.utils import restore_model, save_model
    from emgraph_amd import _lib as L
    D.require_gpu()
    X, n_ent, n_rel = _toy_graph()
    k, eta, epochs, bc, Cs, seed = 8, 3, 3, 4, 16, 3
    rs = np.random.RandomState(5)
    ent0, rel0 = (rs.randn(n_ent, 2 * k) * 0.4).astype(F32), (rs.randn(n_rel, 2 * k) * 0.4).astype(F32)
    m = ComplEx(k=k, eta=eta, epochs=epochs, batches_count=bc, seed=seed, loss="nll", optimizer="adam", optimizer_params={"lr": 0.01},
                embedding_model_params={"shared_negatives": Cs, "corrupt_side": "s,o"}, initializer="constant",
                initializer_params={"entity": ent0, "relation": rel0})
    m.fit(X)
    assert np.all(np.isfinite(m.epoch_losses)) and np.isfinite(m.trained_model_params[0]).all()
    bs = -(-len(X) // bc)
    sizes = [max(0, min(bs, len(X) - i * bs)) for i in range(bc)]
    assert m.negative_sampling_stats == {"rows": epochs * sum(ref.n_chunks(b_, Cs) for b_ in sizes) * eta, "redrawn": 0, "known_left": 0}
    # the same fit as a loop over the ordinary step with the expanded codes
    tr = Trainer(L.COMPLEX, 2 * k, 1.0, ent0, rel0, eta, loss="nll", optimizer="adam", optimizer_params={"lr": 0.01},
                 corrupt_sides=["s,o"], batches_count=bc, seed=seed, fused=False, inplace=False, pipeline=False)
    tr.set_training_set(X.astype(np.int32), bs)
    losses = []
    for epoch in range(1, epochs + 1):
        for b in range(1, bc + 1):
            nb = sizes[b - 1]
            G = ref.n_chunks(nb, Cs)
            cc = D.corrupt_codes(G, eta, L.SIDE_SO, n_ent, "cuda", seed=seed, counter=(epoch - 1) * bc + (b - 1))
            codes = D.expand_shared_codes(cc, nb, Cs, eta)
            tr.step((b - 1) * bs, nb, epoch=epoch, batch=b, inj_repl=(codes & 0x7FFFFFFF).contiguous(),
                    inj_mask=(codes < 0).to(torch.int32).contiguous())
        losses.append(tr.read_loss())
    Eo, Ro = tr.tables_numpy()
    np.testing.assert_allclose(m.trained_model_params[0], Eo, **TABLE_TOL)
    np.testing.assert_allclose(m.trained_model_params[1], Ro, **TABLE_TOL)
    np.testing.assert_allclose(m.epoch_losses, losses, **LOSS_TOL)
    # the key travels through save / restore; prediction does not know about it
    path = str(tmp_path / "shared.pkl")
    save_model(m, path)
    r = restore_model(path)
    assert r.embedding_model_params["shared_negatives"] == Cs and r.all_params["embedding_model_params"]["shared_negatives"] == Cs
    np.testing.assert_array_equal(r.predict(X[:20]), m.predict(X[:20]))


@pytest.mark.parametrize("params,err", [
    ({"shared_negatives": 0}, ValueError), ({"shared_negatives": 257}, ValueError), ({"shared_negatives": "16"}, ValueError),
    ({"shared_negatives": 16, "sharding": "batch"}, NotImplementedError),
    ({"shared_negatives": 16, "negative_side_sampling": "bernoulli"}, NotImplementedError),
    ({"shared_negatives": 16, "filter_negatives": True}, NotImplementedError),
    ({"shared_negatives": 16, "negative_type_constraints": True}, NotImplementedError),
])
def test_fit_refuses_on_the_gpu_box_too(params, err):
    from emgraph_amd.models import ComplEx
    X, _, _ = _toy_graph()
    with pytest.raises(err, match="shared_negatives"):
        ComplEx(k=4, eta=2, epochs=1, batches_count=2, embedding_model_params=params).fit(X)


@pytest.mark.parametrize("pool", [7, [3, 5, 8, 13, 21, 34]])
def test_negative_pools_reach_the_chunk_draws(pool):
    """an int pool and an id list go through n_choices / entities_list as in the ordinary step: every replacement of a chunk comes
    from the pool, and the step is still the ordinary step on the expanded codes"""
    _compare_steps("ComplEx", ("s,o",), "nll", "sgd", pool=pool)


def test_fit_with_negative_corruption_entities():
    from emgraph_amd.models import DistMult
    X, _, _ = _toy_graph()
    for nce in (7, [3, 5, 8, 13], "batch"):     # (7 batches of 43 rows and a last one of 42: a batch shorter than the scratch's)
        m = DistMult(k=8, eta=2, epochs=2, batches_count=7, seed=1,
                     embedding_model_params={"shared_negatives": 8, "negative_corruption_entities": nce})
        m.fit(X)
        assert np.all(np.isfinite(m.epoch_losses)) and np.isfinite(m.trained_model_params[0]).all()
