"""Type constraints on the device against tests/_typed_ref.py: emg_eval_count_grouped against counts formed on the host from the
exact kernel's dense score bits (all seven model ids, == on both counters), rank_triples_device(type_constraints=...) against the
per-(relation, side) loop over the entities_subset path (the oracle the typed rank is defined by), the public functions on
briefly fitted models; and typed negatives: the three producers of corruption ids and fit() against the typed draws of the
reference, a sampler without pools (or bound with the first layout's size) against the untyped reference.

Kernel shapes: 700 entities, 6 relations (12 groups); pools of 0, 1, 63, 64, 65, 129 and 700 members (empty, one masked tile, a
tile less one, a whole tile, a tile and one, two tiles and one, every entity); 0, 1, 64, 65 and 130 rows per group, laid out so
that groups straddle the 64-row windows, with rows of group -1 in between; k_int 5 (6 for the complex models), 72 and 200."""
import functools

import numpy as np
import pytest

from tests import _typed_ref as ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32 = np.float32
N_ENT, N_REL = 700, 6
POOL_SIZES = (0, 1, 63, 64, 65, 129, 700, 129, 1, 65, 700, 63)     # per group
ROWS = (65, 1, 64, 65, 130, 0, 1, 64, 130, 0, 65, 130)              # per group
MODELS = ("TRANSE_L1", "TRANSE_L2", "TRANSE_P", "DISTMULT", "COMPLEX", "HOLE", "ROTATE")


def _libs():
    from emgraph_amd import _lib as L
    from emgraph_amd import device as D
    D.require_gpu()
    return L, D


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _kernel_case():
    """(ptr, idx, row_group): the pools and the rows' groups — group order 0..11 with three rows of group -1 after every second
    group and a window (64 rows) of them at the end"""
    rs = np.random.RandomState(5)
    groups = [sorted(rs.choice(N_ENT, size=n, replace=False).tolist()) for n in POOL_SIZES]
    ptr, idx = ref.pools_csr(groups)
    rg = []
    for g, n in enumerate(ROWS):
        rg += [g] * n
        if g % 2:
            rg += [-1] * 3
    rg += [-1] * 64
    return ptr, idx, np.array(rg, dtype=np.int32)


@pytest.mark.parametrize("k_int", [5, 72, 200])
@pytest.mark.parametrize("model", MODELS)
def test_grouped_count_equals_the_host_counts_of_the_dense_bits(model, k_int):
    L, D = _libs()
    model_id = getattr(L, model)
    if model in ("COMPLEX", "HOLE", "ROTATE"):
        k_int += k_int % 2
    scale = {"HOLE": 2.0 / k_int, "TRANSE_P": 3.0}.get(model, 1.0)
    ptr, idx, rg = _kernel_case()
    n_rows = len(rg)
    rs = np.random.RandomState(k_int)
    E = (rs.randn(N_ENT, k_int) * 0.3).astype(F32)
    E[rs.randint(0, N_ENT, 200)] = E[rs.randint(0, N_ENT, 200)]           # copies: candidates that tie
    Qh = (rs.randn(n_rows, k_int) * 0.3).astype(F32)
    Et, Q = cu(E), cu(Qh)
    S = D.eval_scores_dense(model_id, Q, Et, k_int, scale).cpu().numpy()
    col = [int(rs.choice(ref.pool_of(ptr, idx, g))) if g >= 0 and ptr[g + 1] > ptr[g] else int(rs.randint(N_ENT)) for g in rg.tolist()]
    pos_int = ref.cmp_int(S[np.arange(n_rows), col])    # the integer of a member of the row's pool: every typed row has a tie
    want_gt, want_eq = ref.typed_counts(S, pos_int, rg, ptr, idx)
    assert (want_eq > 0).sum() == 650 and (want_eq > 1).sum() > 5 and (want_gt > 0).sum() > n_rows // 2
    assert not want_gt[rg == 0].any() and not want_eq[rg == 0].any() and (rg == 0).sum() == 65    # an empty pool counts nothing
    cnt = torch.stack([torch.full((n_rows,), 7, dtype=torch.int32), torch.full((n_rows,), 3, dtype=torch.int32)]).cuda()
    D.eval_count_grouped(model_id, Q, cu(pos_int), cu(rg), Et, k_int, scale, cu(ptr), cu(idx), cnt[0], cnt[1])
    got = cnt.cpu().numpy().astype(np.int64)
    np.testing.assert_array_equal(got[0] - 7, want_gt)     # (accumulated onto what was there)
    np.testing.assert_array_equal(got[1] - 3, want_eq)


def test_grouped_count_on_unsorted_groups_and_bad_arguments():
    """any order of the groups is correct (the kernel works on runs), ids past the pools' groups are not counted"""
    L, D = _libs()
    ptr, idx, rg = _kernel_case()
    rs = np.random.RandomState(1)
    rg = rg[rs.permutation(len(rg))].copy()
    rg[:5] = 12                                   # >= n_groups: not counted
    k_int, n_rows = 24, len(rg)
    E = (rs.randn(N_ENT, k_int) * 0.3).astype(F32)
    Et, Q = cu(E), cu((rs.randn(n_rows, k_int) * 0.3).astype(F32))
    S = D.eval_scores_dense(L.DISTMULT, Q, Et, k_int, 1.0).cpu().numpy()
    pos_int = ref.cmp_int(S[np.arange(n_rows), rs.randint(0, N_ENT, n_rows)])
    want_gt, want_eq = ref.typed_counts(S, pos_int, np.where(rg >= 12, -1, rg), ptr, idx)
    cnt = torch.zeros((2, n_rows), dtype=torch.int32, device="cuda")
    D.eval_count_grouped(L.DISTMULT, Q, cu(pos_int), cu(rg), Et, k_int, 1.0, cu(ptr), cu(idx), cnt[0], cnt[1])
    np.testing.assert_array_equal(cnt.cpu().numpy()[0], want_gt)
    np.testing.assert_array_equal(cnt.cpu().numpy()[1], want_eq)
    with pytest.raises(L.EmgError, match="EMG_ROTATE"):
        D.eval_count_grouped(L.ROTATE, Q, cu(pos_int), cu(rg), Et, 23, 1.0, cu(ptr), cu(idx), cnt[0], cnt[1])
    with pytest.raises(L.EmgError, match="unknown model"):
        D.eval_count_grouped(7, Q, cu(pos_int), cu(rg), Et, k_int, 1.0, cu(ptr), cu(idx), cnt[0], cnt[1])


# ---- API parity: the per-(relation, side) loop over the entities_subset path is the oracle ----------------------------------------
@functools.lru_cache(maxsize=None)
def _parity(model):
    """the oracle's ranks of the parity table, computed once: {(side, strategy, filtered): int64 [n]} from
    rank_triples_device(the triples of ONE relation, corrupt_side=side, entities_subset=that pool, precision=0)"""
    L, D = _libs()
    from emgraph_amd.evaluation import FilterIndex, TypeConstraints, rank_triples_device
    case = ref.parity_case()
    model_id = getattr(L, model)
    E, R, T = cu(case["E"]), cu(case["R"]), case["T"]
    findex = FilterIndex(case["F"])
    oracle = {}
    for side in "so":
        for strategy in ("worst", "best", "middle"):
            for filtered in (False, True):
                out = np.zeros(len(T), np.int64)
                for p in range(ref.P_N_REL):
                    rows = np.flatnonzero(T[:, 1] == p)
                    pool = case["groups"][2 * p + (ref.RANGE if side == "o" else ref.DOMAIN)]
                    out[rows] = rank_triples_device(model_id, E, R, ref.P_K_INT, 1.0, T[rows], side, strategy,
                                                    filter_triples=findex if filtered else None,
                                                    entities_subset=np.array(pool) if pool else None, precision=0)
                oracle[side, strategy, filtered] = out
    ptr, idx = ref.pools_csr(case["groups"])
    return case, model_id, E, R, findex, TypeConstraints(ptr, idx, ref.P_N_ENT, ref.P_N_REL), oracle


def _oracle_counters(oracle, side):
    """(gt, eq, fgt, feq) of one side from the oracle's best / worst ranks with and without the filter"""
    bu, wu, bf, wf = (oracle[side, s, f] for s, f in (("best", False), ("worst", False), ("best", True), ("worst", True)))
    gt, eq, fgt = bu - 1, wu - bu, bu - bf
    return gt, eq, fgt, (wu - wf) - fgt


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("strategy", ["worst", "best", "middle"])
@pytest.mark.parametrize("corrupt_side", ["s", "o", "s,o", "s+o"])
@pytest.mark.parametrize("model", ["COMPLEX", "TRANSE_L1"])
def test_typed_ranks_equal_the_subset_loop(model, corrupt_side, strategy, filtered):
    L, D = _libs()
    from emgraph_amd.evaluation import rank_triples_device, ranks_from_counts
    case, model_id, E, R, findex, tc, oracle = _parity(model)
    T, n = case["T"], len(case["T"])
    stats = {}
    got = rank_triples_device(model_id, E, R, ref.P_K_INT, 1.0, T, corrupt_side, strategy, filter_triples=findex if filtered else None,
                              query_chunk=96, precision="auto", type_constraints=tc, stats=stats)
    if corrupt_side in ("s", "o"):
        want = oracle[corrupt_side, strategy, filtered]
    elif corrupt_side == "s,o":
        want = np.stack([oracle["s", strategy, filtered], oracle["o", strategy, filtered]], 1)
    else:   # 's+o' adds the two sides' counters: recovered from the oracle's best / worst ranks, and checked on its 'middle' ones
        c = {sd: _oracle_counters(oracle, sd) for sd in "so"}
        for sd in "so":
            gt, eq, fgt, feq = c[sd]
            np.testing.assert_array_equal(ranks_from_counts(gt, eq, fgt, feq, n, sd, "middle"), oracle[sd, "middle", True])
        zero = np.zeros(n, np.int64)
        cat = [np.concatenate([c["o"][i], c["s"][i]]) if (filtered or i < 2) else np.concatenate([zero, zero]) for i in range(4)]
        want = ranks_from_counts(cat[0], cat[1], cat[2], cat[3], n, "s+o", strategy)
    np.testing.assert_array_equal(got, want)
    sizes = np.diff(tc.pool_ptr)
    rg = np.concatenate([tc.row_groups(T[:, 1], ref.RANGE if sd == "o" else ref.DOMAIN) for sd in "os" if sd in corrupt_side])
    assert stats["typed_pairs"] == sizes[rg[rg >= 0]].sum() and stats["typed_groups"] == len(set(rg[rg >= 0].tolist()))
    for precision in (0, 2):
        np.testing.assert_array_equal(rank_triples_device(model_id, E, R, ref.P_K_INT, 1.0, T, corrupt_side, strategy,
                                                          filter_triples=findex if filtered else None, precision=precision,
                                                          type_constraints=tc), got)


@pytest.mark.parametrize("model", ["COMPLEX", "TRANSE_L1"])
def test_parity_is_not_vacuous(model):
    """typed ranks differ from the untyped ones on at least a quarter of the rows; the filter changes a typed rank; and the device
    ranks are the host chain's (tests/test_type_constraints_host.py asserts the same two conditions on the host reference)"""
    L, D = _libs()
    from emgraph_amd.evaluation import rank_triples_device, ranks_from_counts
    case, model_id, E, R, findex, tc, oracle = _parity(model)
    T, n = case["T"], len(case["T"])
    typed = rank_triples_device(model_id, E, R, ref.P_K_INT, 1.0, T, "s,o", "worst", type_constraints=tc)
    untyped = rank_triples_device(model_id, E, R, ref.P_K_INT, 1.0, T, "s,o", "worst")
    typed_f = rank_triples_device(model_id, E, R, ref.P_K_INT, 1.0, T, "s,o", "worst", filter_triples=findex, type_constraints=tc)
    assert (typed != untyped).mean() >= 0.25
    assert (typed_f != typed).any()
    c = np.concatenate([ref.host_side_counts(model_id, case, sd, True, True) for sd in "os"], axis=1)
    np.testing.assert_array_equal(typed_f, ranks_from_counts(c[0], c[1], c[2], c[3], n, "s,o", "worst"))


@pytest.mark.parametrize("name", ["ComplEx", "RotatE"])
def test_evaluate_performance_with_type_constraints(name):
    L, D = _libs()
    from emgraph_amd import models
    from emgraph_amd.evaluation import FilterIndex, TypeConstraints, evaluate_performance, to_idx
    case = ref.parity_case()
    lab = lambda A: np.stack([np.char.add("e", A[:, 0].astype(str)), np.char.add("r", A[:, 1].astype(str)),   # noqa: E731
                              np.char.add("e", A[:, 2].astype(str))], 1)
    G, T = lab(case["G"]), lab(case["T"])
    m = getattr(models, name)(k=8, eta=2, epochs=2, batches_count=2, seed=3, optimizer="adam", optimizer_params={"lr": 0.01})
    m.fit(G)
    T = T[np.isin(T[:, 0], G[:, [0, 2]]) & np.isin(T[:, 2], G[:, [0, 2]])]
    tc = TypeConstraints.from_triples(G, m)
    assert tc.n_ent == len(m.ent_to_idx) and (np.diff(tc.pool_ptr) > 0).all()
    ranks = np.asarray(evaluate_performance(T, m, filter_triples=np.concatenate([G, T]), type_constraints=tc))
    Ti, Fi = to_idx(T, m.ent_to_idx, m.rel_to_idx), to_idx(np.concatenate([G, T]), m.ent_to_idx, m.rel_to_idx)
    np.testing.assert_array_equal(ranks, m.get_ranks_idx(Ti, filter_idx=FilterIndex(Fi), type_constraints=tc))
    plain = np.asarray(evaluate_performance(T, m, filter_triples=np.concatenate([G, T])))
    assert ranks.shape == plain.shape == (len(T), 2) and (ranks <= plain).all() and (ranks < plain).any() and ranks.min() >= 1
    # the typed rank of one triple is the subset path's
    s, p, o = (int(v) for v in Ti[0])
    one = m.get_ranks_idx(Ti[:1], filter_idx=FilterIndex(Fi), corrupt_side="o", corruption_entities=tc.pool(p, ref.RANGE))
    assert one[0] == ranks[0, 1]


# ---- typed negatives: the three producers of corruption ids against tests/_typed_ref.py ------------------------------------------------
from tests import _negsample_ref as nref                                                          # noqa: E402
from tests.test_negative_sampling import (B, COUNTER0, ETA, SEED, check_prepared, fit_cfg, prepare,   # noqa: E402
                                          record_negatives)

S_SETTINGS = [("uniform", False), ("bernoulli", False), ("uniform", True)]     # pools alone, + Bernoulli, + filter
S_SIDES = [["s,o"], ["s", "o"]]
RETRIES = 4


class BoundPools:
    """a sampler bound for the duration of a ``with`` block: ``pools`` False binds none, ``size`` the structure size handed over"""

    def __init__(self, case, side, flt, n_ent, pools=True, size=None):
        from emgraph_amd import negative_sampling as NS
        L, self.d = _libs()
        self.kw = dict(keep_thr=cu(case["thr"].view(np.int32)) if side == "bernoulli" else None,
                       known_keys=cu(NS.known_triple_keys(case["X"], n_ent, ref.S_N_REL)) if flt else None, retries=RETRIES,
                       stats=torch.zeros(4 if pools else 3, dtype=torch.int64, device="cuda"), size=size)
        if pools:
            self.kw.update(pool_ptr=cu(case["ptr"]), pool_idx=cu(case["idx"]))
        self.n_ent = n_ent

    def __enter__(self):
        self.d.sampler_bind(self.n_ent, ref.S_N_REL, **self.kw)
        return self

    def __exit__(self, *exc):
        self.d.sampler_unbind()

    def stats(self):
        torch.cuda.synchronize()
        r = self.kw["stats"].cpu().numpy()
        self.kw["stats"].zero_()
        return dict(zip(("rows", "redrawn", "known_left", "typed_rows"), (int(v) for v in r)))


@pytest.mark.parametrize("sides", S_SIDES, ids=lambda s: "|".join(s))
@pytest.mark.parametrize("setting", S_SETTINGS, ids=str)
def test_typed_draws_of_the_three_producers_equal_the_reference(setting, sides):
    """emg_corrupt_codes_sampled (with two positives whose relation id is out of range: they draw untyped), emg_prepare_batch's
    counting form on the table of 1200 rows and its bucket form on the tall one: codes, destinations and the four counts"""
    L, D = _libs()
    side, flt = setting
    case = ref.sampler_case()
    ptr, idx, xb = case["ptr"], case["idx"], case["xb"]
    kt, known = (case["thr"] if side == "bernoulli" else None), (case["known"] if flt else None)
    assert sorted(set(np.diff(ptr).tolist())) == [0, 1, 2, 1000] and len(xb) == B
    for n_ent in (ref.S_N_ENT, nref.N_ENT_B):
        want = ref.sample_batch_typed(xb, ETA, sides, SEED, COUNTER0, n_ent, ptr, idx, ref.S_N_REL, kt, known, RETRIES)
        what = str((setting, sides, n_ent))
        for part in want["parts"]:
            # every replacement from a non-empty pool is a member of it; the untyped draw would have left the pool on >= 30 % of the rows
            for r in np.flatnonzero(part["typed"]).tolist():
                g = 2 * int(xb[part["at"][r], 1]) + int(part["keep"][r])
                assert int(part["repl"][r]) in case["groups"][g], what
            assert ref.outside_pool_share(part, xb, ptr, idx, ref.S_N_REL) >= 0.30, what
        assert 0 < want["stats"]["typed_rows"] < want["stats"]["rows"], what   # typed rows and rows of the unconstrained side
        if flt:
            assert want["stats"]["redrawn"] > 50 and want["stats"]["known_left"] > 10, what
        with BoundPools(case, side, flt, n_ent) as b:
            if n_ent == ref.S_N_ENT:
                odd = xb.copy()
                odd[5, 1], odd[17, 1] = 9, -1                               # relation ids out of range
                pos_t = cu(odd.astype(np.int32))
                n_typed = 0
                for sd, s in enumerate(sides):
                    w = ref.sample_side_typed(odd, ETA, s, SEED, COUNTER0 + sd, n_ent, ptr, idx, ref.S_N_REL, kt, known, RETRIES)
                    assert not w["typed"][5::B].any() and not w["typed"][17::B].any()
                    got = D.corrupt_codes_sampled(pos_t, ETA, L.SIDE_IDS[s], n_ent, seed=SEED, counter=COUNTER0 + sd)
                    np.testing.assert_array_equal(got.cpu().numpy(), w["codes"], err_msg=what)
                    n_typed += int(w["typed"].sum())
                assert b.stats()["typed_rows"] == n_typed, what
            bucket = n_ent == nref.N_ENT_B
            check_prepared(prepare(D, xb, sides, n_ent, n_ent, None, grouping="bucket" if bucket else None), want["codes"], xb, what,
                           bucket=bucket)
            assert b.stats() == want["stats"], what
    assert not D.sampler_bound()


@pytest.mark.parametrize("size", [None, "v1"])
def test_a_sampler_without_pools_draws_as_before(size):
    """bound with NULL pools, and bound with the structure size of the first layout: the untyped reference's codes and three counts"""
    L, D = _libs()
    case = ref.sampler_case()
    xb, sides = case["xb"], ["s,o"]
    pos_t = cu(xb.astype(np.int32))
    want = nref.sample_batch(xb, ETA, sides, SEED, COUNTER0, ref.S_N_ENT, None, case["thr"], case["known"], RETRIES)
    typed = ref.sample_batch_typed(xb, ETA, sides, SEED, COUNTER0, ref.S_N_ENT, case["ptr"], case["idx"], ref.S_N_REL, case["thr"],
                                   case["known"], RETRIES)
    assert (want["codes"] != typed["codes"]).mean() > 0.3                  # (the pools would have changed the draws)
    with BoundPools(case, "bernoulli", True, ref.S_N_ENT, pools=False, size=L.SAMPLER_SIZE_V1 if size == "v1" else None) as b:
        got = D.corrupt_codes_sampled(pos_t, ETA, L.SIDE_IDS["s,o"], ref.S_N_ENT, seed=SEED, counter=COUNTER0)
        np.testing.assert_array_equal(got.cpu().numpy(), want["codes"])
        st = b.stats()
        assert {k: st[k] for k in want["stats"]} == want["stats"]
        check_prepared(prepare(D, xb, sides, ref.S_N_ENT, ref.S_N_ENT, None), want["codes"], xb, str(size), bucket=False)
    with pytest.raises(ValueError, match="no room"):
        D.sampler_bind(ref.S_N_ENT, ref.S_N_REL, pool_ptr=cu(case["ptr"]), pool_idx=cu(case["idx"]), size=L.SAMPLER_SIZE_V1)
    assert not D.sampler_bound()


# ---- fit() with typed negatives --------------------------------------------------------------------------------------------------------
def _fit_graph():
    X = ref.fit_graph()
    ptr, idx = ref.pools_from_triples(X, 3)
    return dict(X=X, n_ent=60, ptr=ptr, idx=idx, thr=nref.keep_thresholds(X, 3), known=nref.known_set(X))


@pytest.mark.parametrize("extra", [{}, {"negative_side_sampling": "bernoulli", "filter_negatives": True}], ids=["pools", "pools+bernoulli+filter"])
def test_fit_trains_on_the_typed_reference_negatives(monkeypatch, extra):
    """negative_type_constraints=True: every step's codes are the typed reference's (pools observed from the training triples), the
    four counts are the reference's, and the default path gives the recorded fit's tables, twice"""
    from tests import _fit_steps as fs
    _libs()
    g = _fit_graph()
    cfg = fit_cfg(g, "DistMult", "pairwise", "sgd", dict(extra, negative_type_constraints=True))
    with monkeypatch.context() as mp:
        rec = record_negatives(mp)
        m1, err = fs._fit(cfg)
    assert err is None
    both = bool(extra)
    steps, tot = ref.fit_reference_typed(g["X"], ETA, ["s,o"], cfg["seed"], 3, 2, 60, g["ptr"], g["idx"], 3, g["thr"] if both else None,
                                         g["known"] if both else None, 4)
    assert len(rec) == len(steps) == 6
    for (spec, codes), (epoch, batch, start, Bn, sb) in zip(rec, steps):
        assert spec == (start, Bn, epoch, batch)
        np.testing.assert_array_equal(codes, sb["codes"], err_msg=str(spec))
    assert m1.negative_sampling_stats == tot and tot["typed_rows"] == tot["rows"] == 2 * ETA * len(g["X"])
    assert not both or (tot["redrawn"] > 400 and tot["known_left"] > 10)
    untyped, _ = nref.fit_reference(g["X"], ETA, ["s,o"], cfg["seed"], 3, 2, 60)
    assert np.mean(np.concatenate([a[4]["codes"] for a in untyped]) != np.concatenate([a[4]["codes"] for a in steps])) > 0.3
    for _ in range(2):
        m2, err2 = fs._fit(cfg)
        assert err2 is None and m2.negative_sampling_stats == tot
        np.testing.assert_array_equal(m1.trained_model_params[0], m2.trained_model_params[0])
        np.testing.assert_array_equal(m1.trained_model_params[1], m2.trained_model_params[1])
        assert m1.epoch_losses == m2.epoch_losses
    # the same pools handed over as an object: the same fit
    from emgraph_amd.evaluation import TypeConstraints
    cfg3 = fit_cfg(g, "DistMult", "pairwise", "sgd", dict(extra, negative_type_constraints=TypeConstraints(g["ptr"], g["idx"], 60, 3)))
    m3, err3 = fs._fit(cfg3)
    assert err3 is None and m3.negative_sampling_stats == tot
    np.testing.assert_array_equal(m1.trained_model_params[0], m3.trained_model_params[0])


def test_fit_steps_pass_the_oracle_with_the_typed_negatives(monkeypatch):
    """the host-driven fit: tests/_fit_steps.py's step-by-step check with the oracle's negatives replaced by the typed reference's —
    every step's update and loss inside the intervals of the plain draw's check"""
    from oracle import emgraph_oracle as orc
    from tests import _fit_steps as fs
    _libs()
    g = _fit_graph()
    cfg = fit_cfg(g, "DistMult", "pairwise", "sgd", {"negative_type_constraints": True})

    def typed(xb, entities_list=None, eta=1, corrupt_side="s,o", entities_size=0, seed=0, counter=0):
        return ref.sample_side_typed(xb, eta, corrupt_side, seed, counter, entities_size, g["ptr"], g["idx"], 3)["neg"]

    monkeypatch.setattr(orc, "generate_corruptions_for_fit_philox", typed)
    out = fs.check_step_by_step(cfg, monkeypatch)
    assert out["steps"] == 6 and not out["diverged"]
