"""Sampled ranking on the device against tests/_sampled_ref.py: emg_eval_count_lists against counters formed on the host from the
exact kernel's dense score bits (all seven model ids, TransE-p at orders 3 and inf, == on both counters) and against
emg_eval_filter_count fed the same lists; emg_eval_draw_candidates against the host restatement, id for id; and the public functions
on one-epoch models of every class against the loop of single-triple entities_subset calls.

Kernel shapes: 300 entities (a few rows duplicated: exact ties); k_int 5, 16, 36, 130 (RotatE 6, 34, 130 and 40: the width at which
its rows are staged); entity rows of stride k_int + 3 (read per lane) and of a multiple of 4 (staged through LDS); 1, 7 and 130 query
rows (130: more than one workgroup, lists split over waves at 1 and 7); lists of 1, 63, 64, 65 and 200 entries (one batch less one,
a whole batch, a batch and one, four batches) with duplicates, -1, n_ent, 2^31 - 1, a row that is all padding and the true entity."""
import functools

import numpy as np
import pytest

from tests import _sampled_ref as ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32 = np.float32
EINVAL = -1      # EMG_EINVAL
N_ENT = 300
VARIANTS = (("TRANSE_L1", 1.0), ("TRANSE_L2", 1.0), ("TRANSE_P", 3.0), ("TRANSE_P", float("inf")), ("DISTMULT", 1.0), ("COMPLEX", 1.0),
            ("HOLE", None), ("ROTATE", 1.0))
ROWS, WIDTHS, PAD = (1, 7, 130), (1, 63, 64, 65, 200), 3


def _libs():
    from emgraph_amd import _lib as L
    from emgraph_amd import device as D
    D.require_gpu()
    return L, D


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _widths(model):
    return (6, 34, 40, 130) if model == "ROTATE" else (5, 16, 36, 130)


def _tables(k_int, ld_ent, seed):
    """(E [300, ld_ent] float32 N(0, 1) with 40 duplicated rows, Q [130, k_int + 5], the true entity per row)"""
    rs = np.random.RandomState(seed)
    E = rs.randn(N_ENT, ld_ent).astype(F32)
    src, dst = rs.choice(N_ENT, size=(2, 40), replace=False)
    E[dst] = E[src]                                        # exact ties
    Q = rs.randn(max(ROWS), k_int + 5).astype(F32)
    true = rs.randint(0, N_ENT, max(ROWS))
    true[::3] = dst[rs.randint(0, 40, len(true[::3]))]     # a third of the true entities have a copy elsewhere in the table
    return E, Q, true, dict(zip(dst.tolist(), src.tolist()))


def _lists(rs, n, K, true, copy_of):
    """int32 [n, K + PAD]: ids with replacement, a tenth of the entries padding (-1, n_ent, 2^31 - 1), the true entity (and its copy)
    planted in half of the rows, one row all padding; the PAD columns behind the list hold entity ids that must not be counted"""
    cand = rs.randint(0, N_ENT, size=(n, K + PAD)).astype(np.int32)
    pad = rs.rand(n, K) < 0.1
    cand[:, :K][pad] = rs.choice(np.array([-1, N_ENT, 2 ** 31 - 1], np.int32), size=int(pad.sum()))
    for r in range(0, n, 2):
        cand[r, rs.randint(K)] = true[r]
        if K > 1 and int(true[r]) in copy_of:
            cand[r, (np.flatnonzero(cand[r, :K] == true[r])[0] + 1) % K] = copy_of[int(true[r])]
    if n > 3:
        cand[3, :K] = np.array([-1, N_ENT, 2 ** 31 - 1], np.int32)[np.arange(K) % 3]
    return cand


def _exclusions(rs, cand, K, true, kind):
    """(ptr int64 [n + 1], idx int32) ascending per row — 'some': every second row empty, the others a random set with the true
    entity and a few of the row's own candidates; 'all': every in-range id of the row's list"""
    rows = []
    for r in range(len(cand)):
        ids = cand[r, :K]
        own = ids[(ids >= 0) & (ids < N_ENT)]
        if kind == "all":
            rows.append(np.unique(own))
        elif r % 2:
            rows.append(np.zeros(0, np.int32))
        else:
            rows.append(np.unique(np.concatenate([rs.randint(0, N_ENT, 12), [true[r]], own[:max(1, len(own) // 3)]])))
    ptr = np.zeros(len(cand) + 1, np.int64)
    np.cumsum([len(x) for x in rows], out=ptr[1:])
    return ptr, (np.concatenate(rows) if rows else np.zeros(0)).astype(np.int32)


@pytest.mark.parametrize("width", range(4))
@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: "%s-%s" % (v[0], v[1]))
def test_list_count_equals_the_host_counts_of_the_dense_bits(variant, width):
    L, D = _libs()
    model, scale0 = variant
    model_id = getattr(L, model)
    seen = {"gt": 0, "eq": 0, "skipped": 0, "excluded_rows": 0, "launches": 0}
    for k_int in _widths(model)[width:width + 1]:
        scale = 2.0 / k_int if model == "HOLE" else scale0
        for ld_ent in (k_int + 3, (k_int + 3) // 4 * 4 + 4):
            E, Qh, true, copy_of = _tables(k_int, ld_ent, seed=1000 * k_int + ld_ent)
            Et, Q = cu(E), cu(Qh)
            S = D.eval_scores_dense(model_id, Q, Et, k_int, scale).cpu().numpy()
            ci = ref.cmp_int(S)
            pos_all = ci[np.arange(len(true)), true]
            rs = np.random.RandomState(k_int + ld_ent)
            for n in ROWS:
                pos_int = pos_all[:n].copy()
                for K in WIDTHS:
                    cand = _lists(rs, n, K, true, copy_of)
                    cand_d = cu(cand)
                    assert cand_d.stride(0) == K + PAD
                    for kind in (None, "some", "all"):
                        ptr = idx = None
                        if kind:
                            ptr, idx = _exclusions(rs, cand, K, true, kind)
                        want_gt, want_eq, skipped = ref.list_counts(ci[:n], pos_int, cand, K, N_ENT, ptr, idx)
                        cnt = torch.stack([torch.full((n,), 7, dtype=torch.int32), torch.full((n,), 3, dtype=torch.int32)]).cuda()
                        D.eval_count_lists(model_id, Q[:n], cu(pos_int), Et, k_int, scale, cand_d, cnt[0], cnt[1],
                                           excl_ptr=cu(ptr) if kind else None, excl_idx=cu(idx) if kind else None, n_cand=K)
                        got = cnt.cpu().numpy().astype(np.int64)
                        where = (model, scale, k_int, ld_ent, n, K, kind)
                        np.testing.assert_array_equal(got[0] - 7, want_gt, err_msg=str(where))     # (accumulated onto what was there)
                        np.testing.assert_array_equal(got[1] - 3, want_eq, err_msg=str(where))
                        if kind == "all":
                            assert not want_gt.any() and not want_eq.any() and (skipped == K).all()
                        else:
                            seen["gt"] += int((want_gt > 0).sum())
                            seen["eq"] += int((want_eq > 0).sum())
                            seen["skipped"] += int(skipped.sum())
                            seen["excluded_rows"] += int(kind == "some" and (want_eq[::2] < ref.list_counts(ci[:n], pos_int, cand, K, N_ENT)[1][::2]).any())
                        seen["launches"] += 1
    print("list count %s k_int=%s on %s: %s" % (model, _widths(model)[width], torch.cuda.get_device_name(), seen))
    # the expectation itself is not vacuous: rows that count, rows that tie, entries skipped, an exclusion that removed a tie
    assert seen["gt"] > 250 and seen["eq"] > 25 and seen["skipped"] > 250 and seen["excluded_rows"] > 1, seen
    assert seen["launches"] == 2 * len(ROWS) * len(WIDTHS) * 3


@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: "%s-%s" % (v[0], v[1]))
def test_list_count_equals_filter_count_on_the_same_lists_and_a_second_call_doubles(variant):
    """lists of in-range ids, no exclusion: the counters are what emg_eval_filter_count adds for the lists as its CSR, bit for bit"""
    L, D = _libs()
    model, scale = variant
    model_id = getattr(L, model)
    for k_int in ((34, 40) if model == "ROTATE" else (36, 130)):
        scale = 2.0 / k_int if model == "HOLE" else scale
        for ld_ent in (k_int + 3, (k_int + 3) // 4 * 4 + 4):
            E, Qh, true, _ = _tables(k_int, ld_ent, seed=k_int + ld_ent)
            Et, Q = cu(E), cu(Qh)
            n, K = 130, 65
            rs = np.random.RandomState(k_int)
            cand = rs.randint(0, N_ENT, size=(n, K)).astype(np.int32)
            cand[np.arange(n), rs.randint(0, K, n)] = true[:n]
            pos_int = cu(ref.cmp_int(D.eval_scores_dense(model_id, Q, Et, k_int, scale).cpu().numpy()[np.arange(n), true[:n]]))
            a = torch.zeros((2, n), dtype=torch.int32, device="cuda")
            b = torch.zeros((2, n), dtype=torch.int32, device="cuda")
            D.eval_count_lists(model_id, Q, pos_int, Et, k_int, scale, cu(cand), a[0], a[1])
            D.eval_filter_count(model_id, Q, pos_int, Et, 0, k_int, scale, cu(np.arange(n + 1, dtype=np.int64) * K), cu(cand.reshape(-1)),
                                b[0], b[1])
            assert torch.equal(a, b) and int((a[1] > 0).sum()) == n and int((a[0] > 0).sum()) > n // 2
            D.eval_count_lists(model_id, Q, pos_int, Et, k_int, scale, cu(cand), a[0], a[1])
            assert torch.equal(a, 2 * b)


def test_list_count_refuses_bad_arguments_and_writes_nothing():
    L, D = _libs()
    lib = L.load()
    rs = np.random.RandomState(0)
    n, K, k_int = 9, 20, 16
    Et, Q = cu(rs.randn(N_ENT, k_int).astype(F32)), cu(rs.randn(n, k_int).astype(F32))
    cand, pos = cu(rs.randint(0, N_ENT, (n, K)).astype(np.int32)), cu(np.zeros(n, np.int32))
    ptr, idx = cu(np.zeros(n + 1, np.int64)), cu(np.zeros(1, np.int32))
    cnt = torch.full((2, n), 5, dtype=torch.int32, device="cuda")

    def call(model=L.DISTMULT, ldq=k_int, n_rows=n, n_ent=N_ENT, ld_ent=k_int, ld_cand=K, n_cand=K, xp=None, xi=None, k=k_int, scale=1.0):
        return lib.emg_eval_count_lists(model, Q.data_ptr(), ldq, pos.data_ptr(), n_rows, Et.data_ptr(), n_ent, ld_ent, cand.data_ptr(),
                                        ld_cand, n_cand, xp, xi, k, scale, cnt[0].data_ptr(), cnt[1].data_ptr(), None)

    bad = [dict(model=7), dict(model=-1), dict(ldq=k_int - 1), dict(ld_ent=k_int - 1), dict(ld_cand=K - 1), dict(model=L.ROTATE, k=15),
           dict(model=L.TRANSE_P, scale=0.0), dict(model=L.TRANSE_P, scale=-2.0), dict(n_ent=1 << 31), dict(xp=ptr.data_ptr()),
           dict(xi=idx.data_ptr()), dict(k=0), dict(n_rows=-1), dict(n_cand=-1)]
    for kw in bad:
        assert call(**kw) == EINVAL, kw
    assert call(n_rows=0) == 0 and call(n_cand=0) == 0            # nothing to do: OK, nothing launched
    torch.cuda.synchronize()
    assert (cnt == 5).all()
    assert call() == 0                                              # the same arguments, unspoilt, do count
    once = cnt.clone()
    assert (once[0] > 5).any() and (once >= 5).all() and (once[0] + once[1] <= 10 + K).all()
    assert call(xp=ptr.data_ptr(), xi=idx.data_ptr()) == 0          # (exclusion lists that are all empty: the same counts again)
    torch.cuda.synchronize()
    assert torch.equal(cnt - 5, 2 * (once - 5))
    with pytest.raises(ValueError, match="come together"):
        D.eval_count_lists(L.DISTMULT, Q, pos, Et, k_int, 1.0, cand, cnt[0], cnt[1], excl_ptr=ptr)


@pytest.mark.parametrize("n_ent", [1, 300, 2 ** 31 - 1])
def test_drawn_lists_equal_the_host_restatement(n_ent):
    L, D = _libs()
    lib = L.load()
    n_q, q_offset, seed = 37, 1000003, 0x9E3779B97F4A7C15
    for side_mode in range(4):
        n_rows = 2 * n_q if side_mode >= 2 else n_q
        for K in (1, 5, 64):
            buf = torch.full((n_rows, K + 2), -7, dtype=torch.int32, device="cuda")
            assert lib.emg_eval_draw_candidates(n_q, q_offset, side_mode, K, n_ent, seed, buf.data_ptr(), K + 2, None) == 0
            got = buf.cpu().numpy()
            np.testing.assert_array_equal(got[:, :K], ref.draw_rows(n_q, q_offset, side_mode, K, n_ent, seed))
            assert (got[:, K:] == -7).all()                      # nothing behind the list is written
            np.testing.assert_array_equal(D.eval_draw_candidates(n_q, q_offset, side_mode, K, n_ent, seed, "cuda").cpu().numpy(), got[:, :K])
    buf = torch.full((4, 4), -7, dtype=torch.int32, device="cuda")
    for kw in (dict(side=4), dict(side=-1), dict(n_ent=0), dict(n_ent=1 << 31), dict(ld=3), dict(off=-1)):
        assert lib.emg_eval_draw_candidates(4, kw.get("off", 0), kw.get("side", 0), 4, kw.get("n_ent", 9), 1, buf.data_ptr(), kw.get("ld", 4),
                                            None) == EINVAL, kw
    assert lib.emg_eval_draw_candidates(0, 0, 0, 4, 9, 1, buf.data_ptr(), 4, None) == 0
    torch.cuda.synchronize()
    assert (buf == -7).all()


# ---- the public functions: the loop of single-triple entities_subset calls is the oracle ----------------------------------------------
MODELS = (("TransE", {"norm": 1}), ("TransE", {"norm": 2}), ("TransE", {"norm": 3}), ("DistMult", {}), ("ComplEx", {}), ("HolE", {}),
          ("RotatE", {}))
K_API = 20


def _labels(A):
    return np.stack([np.char.add("e", A[:, 0].astype(str)), np.char.add("r", A[:, 1].astype(str)), np.char.add("e", A[:, 2].astype(str))], 1)


@functools.lru_cache(maxsize=None)
def _fitted(name, params):
    """(model, train labels, test labels, test ids, filter ids, {'s' / 'o': distinct candidate ids [n, K_API]}, oracle) — the oracle:
    {(side, strategy, filtered): int64 [n]} from get_ranks_idx(ONE triple, corrupt_side=side, corruption_entities=its list)"""
    _libs()
    from emgraph_amd import models
    from emgraph_amd.evaluation import FilterIndex, to_idx
    G, T = ref.toy_graph()
    T = T[np.isin(T[:, 0], G[:, [0, 2]]) & np.isin(T[:, 2], G[:, [0, 2]])]
    Gl, Tl = _labels(G), _labels(T)
    m = getattr(models, name)(k=8, eta=2, epochs=1, batches_count=2, seed=3, optimizer="adam", optimizer_params={"lr": 0.01},
                              embedding_model_params=dict(params))
    m.fit(Gl)
    Ti = to_idx(Tl, m.ent_to_idx, m.rel_to_idx)
    Fi = to_idx(np.concatenate([Gl, Tl]), m.ent_to_idx, m.rel_to_idx)
    rs = np.random.RandomState(8)
    n_ent = len(m.ent_to_idx)
    lists = {sd: np.stack([rs.permutation(n_ent)[:K_API] for _ in range(len(Ti))]) for sd in "so"}
    for i in range(0, len(Ti), 2):                       # the true entity in half of the lists
        for sd, col in (("s", 0), ("o", 2)):
            if Ti[i, col] not in lists[sd][i]:
                lists[sd][i, i % K_API] = Ti[i, col]
    findex = FilterIndex(Fi)
    oracle = {}
    for side in "so":
        for strategy in ("worst", "best", "middle"):
            for filtered in (False, True):
                oracle[side, strategy, filtered] = np.array([
                    m.get_ranks_idx(Ti[i:i + 1], filter_idx=findex if filtered else None, corrupt_side=side, ranking_strategy=strategy,
                                    corruption_entities=lists[side][i])[0] for i in range(len(Ti))], dtype=np.int64)
    return m, Gl, Tl, Ti, Fi, lists, oracle


def _oracle_counters(oracle, side, filtered):
    """(gt, eq) of the entries that survive, from the oracle's best / worst ranks (ranks are 1 + counters under both strategies)"""
    best, worst = oracle[side, "best", filtered], oracle[side, "worst", filtered]
    return best - 1, worst - best


@pytest.mark.parametrize("model", MODELS, ids=lambda v: v[0] + "".join("-%s" % x for x in v[1].values()))
def test_evaluate_performance_with_lists_equals_the_subset_loop(model):
    L, D = _libs()
    from emgraph_amd.evaluation import evaluate_performance, hits_at_n_score, mrr_score
    m, Gl, Tl, Ti, Fi, lists, oracle = _fitted(model[0], tuple(sorted(model[1].items())))
    inv = np.empty(len(m.ent_to_idx), dtype=object)
    for label, i in m.ent_to_idx.items():
        inv[i] = label
    cands = {sd: inv[lists[sd]].astype(str) for sd in "so"}
    rounding_differs = 0
    for filtered in (False, True):
        F = np.concatenate([Gl, Tl]) if filtered else None
        for strategy in ("worst", "best", "middle"):
            want = {}
            for sd in "so":
                gt, eq = _oracle_counters(oracle, sd, filtered)
                want[sd] = ref.cmp_counts(gt, eq, strategy) + 1          # 1 + cmp over the surviving entries
                # ... which IS the subset call's rank, except where 'middle' rounds the list's and the filter's ties separately:
                # ceil((eq - feq) / 2) against ceil(eq / 2) - ceil(feq / 2), eq the ties of the whole list, feq those the filter removes
                eq_all = _oracle_counters(oracle, sd, False)[1]
                feq = eq_all - eq
                same_rounding = (eq + 1) // 2 == (eq_all + 1) // 2 - (feq + 1) // 2
                same = want[sd] == oracle[sd, strategy, filtered]
                if strategy == "middle" and filtered:
                    np.testing.assert_array_equal(same, same_rounding)
                else:
                    assert same.all()
                rounding_differs += int((~same).sum())
            for corrupt_side in ("s", "o", "s,o", "s+o"):
                got = np.asarray(evaluate_performance(Tl, m, filter_triples=F, corrupt_side=corrupt_side, ranking_strategy=strategy,
                                                      candidates={sd: cands[sd] for sd in ref.SIDES_OF[corrupt_side]}))
                if corrupt_side in ("s", "o"):
                    exp = want[corrupt_side]
                elif corrupt_side == "s,o":
                    exp = np.stack([want["s"], want["o"]], 1)
                else:
                    c = {sd: _oracle_counters(oracle, sd, filtered) for sd in "so"}
                    exp = ref.cmp_counts(c["o"][0] + c["s"][0], c["o"][1] + c["s"][1], strategy) + 1
                np.testing.assert_array_equal(got, exp, err_msg=str((filtered, strategy, corrupt_side)))
                assert got.min() >= 1 and got.max() <= (2 * K_API if corrupt_side == "s+o" else K_API) + 1
                assert 0.0 < mrr_score(got) <= 1.0 and 0.0 <= hits_at_n_score(got, 3) <= 1.0
    print("%s: %d test triples, oracle ranks %d..%d, 'middle' roundings that differ: %d" % (model[0], len(Ti), min(v.min() for v in oracle.values()),
                                                                                       max(v.max() for v in oracle.values()), rounding_differs))
    assert rounding_differs <= len(Ti)           # (two sides x one strategy x one filter setting could differ at all)
    assert (oracle["o", "worst", True] != oracle["o", "worst", False]).any()      # the filter excluded something


@pytest.mark.parametrize("model", [MODELS[0], MODELS[4], MODELS[6]], ids=lambda v: v[0])
def test_drawn_candidates_equal_the_restated_lists_whatever_the_chunk(model):
    L, D = _libs()
    from emgraph_amd.evaluation import FilterIndex, evaluate_performance, rank_triples_device
    m, Gl, Tl, Ti, Fi, _, _ = _fitted(model[0], tuple(sorted(model[1].items())))
    n_ent, K, seed = len(m.ent_to_idx), 16, 77
    findex = FilterIndex(Fi)
    for corrupt_side in ("s", "o", "s,o", "s+o"):
        drawn = ref.draw_candidates(len(Ti), corrupt_side, K, n_ent, seed)
        got = m.get_ranks_idx(Ti, filter_idx=findex, corrupt_side=corrupt_side, candidates=K, candidates_seed=seed)
        np.testing.assert_array_equal(got, m.get_ranks_idx(Ti, filter_idx=findex, corrupt_side=corrupt_side, candidates=drawn))
        assert got.min() >= 1 and got.max() <= (2 * K if corrupt_side == "s+o" else K) + 1
        ent, rel = m._device_tables()
        for chunk in (4, 4096):
            stats = {}
            np.testing.assert_array_equal(rank_triples_device(m._model_id(), ent, rel, m.internal_k, m._scale(), Ti, corrupt_side, "worst",
                                                              filter_triples=findex, query_chunk=chunk, candidates=K, candidates_seed=seed,
                                                              stats=stats), got)
            assert stats["list_pairs"] == (1 if corrupt_side in ("s", "o") else 2) * len(Ti) * K and stats["count_ms"] > 0.0
            assert stats["count_launches"] == -(-len(Ti) // chunk)
    np.testing.assert_array_equal(np.asarray(evaluate_performance(Tl, m, filter_triples=np.concatenate([Gl, Tl]), candidates=K, candidates_seed=seed)),
                                  m.get_ranks_idx(Ti, filter_idx=findex, candidates=K, candidates_seed=seed))
    other = m.get_ranks_idx(Ti, filter_idx=findex, candidates=K, candidates_seed=seed + 1)
    assert (other != m.get_ranks_idx(Ti, filter_idx=findex, candidates=K, candidates_seed=seed)).any()


def test_early_stopping_against_drawn_candidates_stops_on_the_same_epoch():
    """a learning rate too small to move a rank, the same lists at every check: the criterion never improves, so the fit stops after
    stop_interval checks — on the same epoch in two runs"""
    _libs()
    from emgraph_amd.models import ComplEx
    G, T = ref.toy_graph()
    Gl = _labels(G)
    epochs = []
    for _ in range(2):
        m = ComplEx(k=8, eta=2, epochs=30, batches_count=2, seed=3, optimizer="sgd", optimizer_params={"lr": 1e-12})
        m.fit(Gl, early_stopping=True, early_stopping_params={"x_valid": Gl[:32], "criteria": "mrr", "burn_in": 0, "check_interval": 1,
                                                              "stop_interval": 2, "x_filter": Gl, "candidates": 16, "candidates_seed": 5})
        assert m.is_fitted and m.early_stopping_epoch is not None and m.early_stopping_epoch <= 4
        epochs.append(m.early_stopping_epoch)
    assert epochs[0] == epochs[1]
