"""RotatE exact-fast ranking on the device (csrc/emg_rank_rotate.hip, the RotatE form of emg_eval_rescore_pairs): the band pair
by pair, the counters against the exact kernel's under ==, overflow, the range refusal, the public path, the re-scoring alone.

Shapes (tests/_rotate_fast_ref.py): k in {1, 3, 4, 33, 64, 100} (odd k, k_int no multiple of 4 or 8, an image row narrower than,
equal to and wider than a tile of 8 coordinates), rows in {1, 33, 130} (a second workgroup of query rows with a tail), entities in
{1, 127, 129, 4099} (one candidate, a tile less one, a tile plus one, a second chunk of 32 tiles with a tail).  Tables: normal at
scale 0.3, at 1e-3, entries of 1e-6 beside entries of 100, all zero."""
import numpy as np
import pytest

from tests import _rotate_fast_ref as ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32 = np.float32


def _libs():
    from emgraph_amd import _lib as L
    from emgraph_amd import device as D
    D.require_gpu()
    return L, D


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _images(D, L, Et, Rt, Tt, ki, side=None):
    """(Q, pos_int, scale, Qh, rho_q, q_stats, Eh, e_stats) of a call, by the protocol of ranking.RotateTables"""
    from emgraph_amd.evaluation.ranking import rotate_image_scale
    Q, pos_int = D.eval_build_queries(L.ROTATE, Et, Rt, ki, 1.0, Tt, L.EVAL_O if side is None else side)
    rng = D.eval_rotate_image(Et, ki, 1.0, check=True, image=False)
    assert rng is not None
    s = rotate_image_scale(float(rng[2][1]))
    Eh, _, e_stats = D.eval_rotate_image(Et, ki, s, check=True)
    Qh, rho_q, q_stats = D.eval_rotate_image(Q, ki, s)
    return Q, pos_int, s, Qh, rho_q, q_stats, Eh, e_stats


# ---- 1. the band, pair by pair ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ref.TABLES)
@pytest.mark.parametrize("k", ref.KS)
def test_band_pair_by_pair(k, kind):
    """|A - S| within the band the thresholds assume, in float64, for EVERY pair: S the exact kernel's dense scores, A the dense debug
    form of the prefilter (the same device function as the counting kernel).  Also: the device image equals the host image bit for
    bit, the device rho bounds the float64 residual sum from above (and by no more than 1e-6 of it), the scale is the documented one."""
    L, D = _libs()
    ki, n = 2 * k, k
    worst = 0.0
    for n_ent in ref.ENTS:
        E, R = ref.entity_table(kind, n_ent, ki), ref.relation_table(ki)
        Et, Rt = cu(E), cu(R)
        for rows in ref.ROWS:
            T = ref.triples(rows, n_ent)
            Q, _, s, Qh, rho_q, q_stats, Eh, e_stats = _images(D, L, Et, Rt, cu(T), ki)
            assert s == ref.image_scale(float(np.abs(E).max())) and float(q_stats[2]) == 0.0 and float(e_stats[2]) == 0.0
            # the image and its residuals
            ld = D.eval_rotate_ld(ki)
            for x, xh, rho in ((E, Eh, None), (Q.cpu().numpy(), Qh, rho_q)):
                h, rho_ref = ref.image(x, ki, s)
                assert np.array_equal(xh.cpu().numpy().view(np.uint16), ref.interleaved(h, ki, ld).view(np.uint16))
                if rho is not None:
                    r = rho.cpu().numpy().astype(np.float64)
                    assert np.all(r >= rho_ref) and np.all(r <= rho_ref * (1 + 1e-6) + 1e-300)
            h_e, rho_e = ref.image(E, ki, s)
            assert float(e_stats[0]) >= rho_e.max() and float(e_stats[0]) <= rho_e.max() * (1 + 1e-6) + 1e-300
            assert float(e_stats[1]) == float(np.abs(E).max())
            # the band
            A = D.eval_prefilter_rotate_dense(Qh, Eh, ki, s).cpu().numpy().astype(np.float64)
            S = D.eval_scores_dense(L.ROTATE, Q, Et, ki, 1.0).cpu().numpy().astype(np.float64)
            rho = rho_q.cpu().numpy().astype(np.float64)[:, None] + float(e_stats[0])
            lower, upper = ref.chain_bounds(A * s, rho, n, s)
            assert np.all(-S >= lower) and np.all(-S <= upper), (k, kind, n_ent, rows)
            band = np.maximum(upper - A, A - lower)
            assert np.all(np.abs(A + S) <= band)
            if band.max() > 0:
                worst = max(worst, float((np.abs(A + S) / np.where(band > 0, band, 1.0)).max()))
    print("k=%d %s: largest |A - S| / band = %.3f" % (k, kind, worst))


# ---- 2. the counters, bit-equal ------------------------------------------------------------------------------------------------------
def _planted(kind, n_ent, ki, rows):
    """table, relations and triples with candidates planted in the band: subjects are rows [0, 4), never planted; where the table
    has room, near-copies of positives' object rows (a few entries moved by 1-3 ulp), exact copies (ties), a positive that is the
    best candidate of its row (planted by the caller from the query row) and one that is the worst"""
    E, R = ref.entity_table(kind, n_ent, ki), ref.relation_table(ki)
    T = ref.triples(rows, n_ent, s_below=4)
    if n_ent >= 127:
        rs = np.random.RandomState(n_ent + ki + rows)
        free = np.setdiff1d(np.arange(8, n_ent), T[:, 2])
        slots = rs.permutation(free)[:48]
        for i, slot in enumerate(slots):
            o = T[i % rows, 2]
            E[slot] = E[o]
            if i % 3:   # 1-3 ulp on a few entries; i % 3 == 0: an exact copy
                cols = rs.randint(0, ki, 3)
                steps, to = rs.randint(1, 4, 3), rs.choice([-np.inf, np.inf], 3).astype(F32)
                v = E[slot, cols]
                for i_step in range(3):
                    v = np.where(i_step < steps, np.nextafter(v, to), v)
                E[slot, cols] = v
        if rows > 1:
            E[T[1, 2]] = F32(4.0) * np.where(np.arange(ki) % 2, F32(1), F32(-1))   # far from every query row: the worst candidate
            T[2:, 2] = np.where(T[2:, 2] == T[1, 2], T[0, 2], T[2:, 2])
    return E, R, T


def _fast_counts(D, L, Q, pos_int, s, Qh, rho_q, q_stats, Eh, e_stats, slab, e0, ki, per_seg=None):
    n_rows, n_cand = Q.shape[0], slab.shape[0]
    thr = D.eval_rotate_thresholds(pos_int, rho_q, ki, s, q_stats, e_stats)
    n_seg = D.eval_prefilter_rotate_segments(n_rows, n_cand)
    per = per_seg if per_seg is not None else min(n_rows, 128) * min(n_cand, 1024)   # room for every pair of a wave
    pairs = torch.empty(n_seg * per, dtype=torch.int64, device="cuda")
    pcount = torch.full((n_seg + 1,), 77, dtype=torch.int32, device="cuda")        # (the call zeroes it)
    cnt = torch.zeros((2, n_rows), dtype=torch.int32, device="cuda")
    D.eval_prefilter_rotate(Qh, thr, Eh[e0:e0 + n_cand], e0, ki, cnt[0], pairs, pcount)
    D.eval_rescore_pairs(L.ROTATE, Q, pos_int, slab, e0, ki, 1.0, pairs, pcount, n_seg, cnt[0], cnt[1], 4)
    return cnt.cpu().numpy(), pcount.cpu().numpy(), pairs


@pytest.mark.parametrize("kind", ref.TABLES)
@pytest.mark.parametrize("k", ref.KS)
def test_counters_equal_the_exact_kernel(k, kind):
    """prefilter + re-scoring == emg_eval_count(EMG_ROTATE, precision 0) on cnt_gt and cnt_eq, on a slab with ent_offset != 0, with
    near-copies, ties, a best and a worst positive planted"""
    L, D = _libs()
    ki = 2 * k
    for n_ent in ref.ENTS:
        for rows in ref.ROWS:
            E, R, T = _planted(kind, n_ent, ki, rows)
            Et, Rt, Tt = cu(E), cu(R), cu(T)
            if n_ent >= 127:   # the best candidate: the positive's row IS the query row (distance 0, pos_int 0)
                Q0, _ = D.eval_build_queries(L.ROTATE, Et, Rt, ki, 1.0, Tt, L.EVAL_O)
                Et[int(T[0, 2])] = Q0[0, :ki]
            Q, pos_int, s, Qh, rho_q, q_stats, Eh, e_stats = _images(D, L, Et, Rt, Tt, ki)
            e0 = 3 if n_ent > 3 else 0
            slab = Et[e0:]
            want = torch.zeros((2, rows), dtype=torch.int32, device="cuda")
            D.eval_count(L.ROTATE, Q, pos_int, slab, ki, 1.0, want[0], want[1])
            got, pcount, _ = _fast_counts(D, L, Q, pos_int, s, Qh, rho_q, q_stats, Eh, e_stats, slab, e0, ki)
            assert pcount[-1] == 0
            assert np.array_equal(got, want.cpu().numpy()), (k, kind, n_ent, rows)
            if n_ent >= 127:
                p = pos_int.cpu().numpy()
                assert p[0] == 0 and got[0, 0] == 0                      # nothing beats the best positive
                if rows > 1 and kind in ("normal", "small"):             # (beside entries of 100 a row of 4s is not far)
                    assert p[1] == p.min() and got[0, 1] + got[1, 1] == slab.shape[0]


def test_undecided_share_on_random_positives():
    """scale 0.3, k = 64, 130 x 4099, random positives: below 10 % undecided (the host emulation of the band gives 2.0-2.4 %: the
    cap only catches a vacuous band)"""
    L, D = _libs()
    ki, n_ent, rows = 128, 4099, 130
    E, R, T = ref.entity_table("normal", n_ent, ki), ref.relation_table(ki), ref.triples(rows, n_ent)
    Et = cu(E)
    Q, pos_int, s, Qh, rho_q, q_stats, Eh, e_stats = _images(D, L, Et, cu(R), cu(T), ki)
    _, pcount, _ = _fast_counts(D, L, Q, pos_int, s, Qh, rho_q, q_stats, Eh, e_stats, Et, 0, ki)
    share = float(pcount[:-1].sum()) / (rows * n_ent)
    print("undecided share: %.4f" % share)
    assert pcount[-1] == 0 and share < 0.10


# ---- 3. overflow -------------------------------------------------------------------------------------------------------------------
def test_overflow_raises_the_flag_and_python_falls_back(monkeypatch):
    L, D = _libs()
    from emgraph_amd.evaluation.ranking import rank_triples_device
    ki, n_ent, rows = 32, 32768, 130
    E, R, T = ref.entity_table("normal", n_ent, ki), ref.relation_table(ki), ref.triples(rows, n_ent)
    Et, Rt = cu(E), cu(R)
    Q, pos_int, s, Qh, rho_q, q_stats, Eh, e_stats = _images(D, L, Et, Rt, cu(T), ki)
    _, pcount, _ = _fast_counts(D, L, Q, pos_int, s, Qh, rho_q, q_stats, Eh, e_stats, Et, 0, ki, per_seg=1)
    assert pcount[-1] != 0 and pcount[:-1].max() <= 1
    want = rank_triples_device(L.ROTATE, Et, Rt, ki, 1.0, T, "s,o", "worst", precision=0)
    monkeypatch.setenv("EMG_PAIR_CAP", "1")   # (64 entries per wave is the floor: far below the undecided set of 128 x 1024 candidates)
    for probe in ("0", "1"):                  # without the probe the tile overflows and is redone; with it the call never starts the mode
        monkeypatch.setenv("EMG_PREFILTER_PROBE", probe)
        stats = {}
        got = rank_triples_device(L.ROTATE, Et, Rt, ki, 1.0, T, "s,o", "worst", precision="auto", stats=stats)
        assert np.array_equal(got, want)
        assert stats["rotate_fast"] is True and stats["fallback"] == 1 and stats.get("pairs", 0) == 0
        assert ("pairs" in stats) == (probe == "0") and stats.get("probe_undecided", 1.0) == 1.0


def test_a_table_of_ties_takes_the_exact_kernel_after_the_probe():
    """entries of 1e-9: every comparison integer is 0, every candidate ties with the positive and none can be decided — the probe sends
    the call to the exact kernel"""
    L, D = _libs()
    from emgraph_amd.evaluation.ranking import RotateTables, rank_triples_device
    ki, n_ent, rows = 32, 32768, 130
    E, R, T = ref.entity_table("normal", n_ent, ki) * F32(1e-8), ref.relation_table(ki), ref.triples(rows, n_ent)
    Et, Rt = cu(E), cu(R)
    tabs = RotateTables(Et, Rt, ki)
    assert tabs.ok and tabs.scale == 2.0 ** 24
    stats = {}
    got = rank_triples_device(L.ROTATE, Et, Rt, ki, 1.0, T, "s,o", "worst", precision="auto", stats=stats, ent_f16=tabs)
    assert np.array_equal(got, rank_triples_device(L.ROTATE, Et, Rt, ki, 1.0, T, "s,o", "worst", precision=0))
    assert (got == got.flat[0]).all() and got.flat[0] >= n_ent - 1   # 'worst': every tie counts against the positive
    assert stats["probe_undecided"] == 1.0 and stats["fallback"] == 1 and "pairs" not in stats and len(tabs.undecided) == 1


# ---- 4. the range refusal ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", ["7e4", "nan"])
def test_range_refusal(bad):
    L, D = _libs()
    from emgraph_amd.evaluation.ranking import RotateTables, rank_triples_device
    ki, n_ent, rows = 32, 32768, 130
    E, R, T = ref.entity_table("normal", n_ent, ki), ref.relation_table(ki), ref.triples(rows, n_ent)
    if bad == "7e4":
        E[777, 5] = 7e4
    else:
        E[777] = np.nan
    Et, Rt = cu(E), cu(R)
    lib = L.load()
    stats3 = torch.empty(3, dtype=torch.float64, device="cuda")
    img = torch.empty((n_ent, D.eval_rotate_ld(ki)), dtype=torch.float16, device="cuda")
    rho = torch.empty(n_ent, dtype=torch.float32, device="cuda")
    rc = lib.emg_eval_rotate_image(Et.data_ptr(), n_ent, Et.stride(0), ki, 1.0, img.data_ptr(), img.stride(0), rho.data_ptr(),
                                   stats3.data_ptr(), 1, None)
    torch.cuda.synchronize()
    assert rc == L.ENOSUP == -3 and float(stats3[2]) != 0.0
    assert torch.isfinite(img.float()).all()            # the image of a refused table is finite all the same
    assert D.eval_rotate_image(Et, ki, 1.0, check=True) is None and not RotateTables(Et, Rt, ki).ok
    stats = {}
    got = rank_triples_device(L.ROTATE, Et, Rt, ki, 1.0, T, "s,o", "worst", filter_triples=T, precision="auto", stats=stats)
    want = rank_triples_device(L.ROTATE, Et, Rt, ki, 1.0, T, "s,o", "worst", filter_triples=T, precision=0)
    assert np.array_equal(got, want) and stats["rotate_fast"] is False and "pairs" not in stats


# ---- 5. the public path ----------------------------------------------------------------------------------------------------------
def _public_case():
    ki, n_ent, rows = 32, 32768, 130      # k = 16: the smallest table 'auto' routes
    E, R = ref.entity_table("normal", n_ent, ki, seed=2), ref.relation_table(ki, seed=2)
    T = ref.triples(rows, n_ent, seed=2)
    rs = np.random.RandomState(5)
    extra = np.stack([np.repeat(T[:, 0], 3), np.repeat(T[:, 1], 3), rs.randint(0, n_ent, 3 * rows)], 1).astype(np.int32)
    return ki, E, R, T, np.concatenate([T, extra])


def test_public_path_auto_equals_exact():
    L, D = _libs()
    from emgraph_amd.evaluation.ranking import FilterIndex, RotateTables, derived_tables, rank_triples_device, resolve_auto_precision
    ki, E, R, T, X = _public_case()
    Et, Rt = cu(E), cu(R)
    assert resolve_auto_precision(L.ROTATE, ki, len(T), E.shape[0]) == 2
    tabs = derived_tables(L.ROTATE, Et, Rt, ki)
    assert isinstance(tabs, RotateTables) and tabs.ok
    findex = FilterIndex(X)
    for filt in (None, findex):
        for strategy in ("worst", "best", "middle"):
            stats = {}
            got = rank_triples_device(L.ROTATE, Et, Rt, ki, 1.0, T, "s,o", strategy, filter_triples=filt, precision="auto", ent_f16=tabs,
                                      stats=stats)
            want = rank_triples_device(L.ROTATE, Et, Rt, ki, 1.0, T, "s,o", strategy, filter_triples=filt, precision=0)
            assert got.shape == (len(T), 2) and np.array_equal(got, want), (filt is not None, strategy)
            assert stats["rotate_fast"] is True and stats["fallback"] == 0 and 0 < stats["pairs"] < 0.1 * 2 * len(T) * E.shape[0]
            assert 0.0 < stats["probe_undecided"] < 0.04
    # without kept tables, and one side
    stats = {}
    got = rank_triples_device(L.ROTATE, Et, Rt, ki, 1.0, T, "o", "worst", precision="auto", stats=stats)
    assert np.array_equal(got, rank_triples_device(L.ROTATE, Et, Rt, ki, 1.0, T, "o", "worst", precision=0)) and stats["rotate_fast"]
    # what stays refused
    for prec in (1, 2):
        with pytest.raises(NotImplementedError, match="RotatE"):
            rank_triples_device(L.ROTATE, Et, Rt, ki, 1.0, T, precision=prec)
    with pytest.raises(NotImplementedError, match="RotatE"):
        rank_triples_device(L.ROTATE, Et, Rt, ki, 1.0, T, precision="auto", shard=(0, 2))


def test_model_path_auto_equals_exact():
    """RotatE.get_ranks_idx / evaluate_performance on a model whose tables are set by hand: 'auto' (the default) equals 0, and the
    fitted model keeps the derived tables"""
    _libs()
    from emgraph_amd.evaluation import evaluate_performance
    from emgraph_amd.evaluation.ranking import FilterIndex, RotateTables
    from emgraph_amd.models import RotatE
    ki, E, R, T, X = _public_case()
    m = RotatE(k=ki // 2, epochs=1, batches_count=1)
    m.ent_to_idx = {"e%05d" % i: i for i in range(len(E))}
    m.rel_to_idx = {"r%d" % i: i for i in range(len(R))}
    m.trained_model_params = [E, R]
    m.is_fitted = True
    assert m._eval_precision() == "auto"
    findex = FilterIndex(X)
    got = m.get_ranks_idx(T, filter_idx=findex)
    kept = m._derived_cache[1]
    assert isinstance(kept, RotateTables) and kept.ok
    m.get_ranks_idx(T[:128], filter_idx=findex)
    assert m._derived_cache[1] is kept
    labels = np.stack([["e%05d" % s for s in T[:, 0]], ["r%d" % p for p in T[:, 1]], ["e%05d" % o for o in T[:, 2]]], 1)
    got_eval = np.asarray(evaluate_performance(labels, m))
    m.embedding_model_params["eval_precision"] = 0
    assert np.array_equal(got, m.get_ranks_idx(T, filter_idx=findex))
    assert np.array_equal(got_eval, np.asarray(evaluate_performance(labels, m)))
    m.embedding_model_params["eval_precision"] = 2
    with pytest.raises(NotImplementedError, match="RotatE"):
        m.get_ranks_idx(T)


# ---- 6. the re-scoring form alone -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (3, 4, 12, 33, 64))
def test_rescore_pairs_rotate_alone(k):
    """hand-made pair lists — an empty segment, a full one, a partial one, one past a batch of 64 — through emg_eval_rescore_pairs
    with EMG_ROTATE against host counting on emg_eval_scores_dense's bits; k = 4, 12, 64: the staged form (k_int % 8 == 0; 12: a slice
    with a tail), 3 and 33: the plain one; a slab offset"""
    L, D = _libs()
    ki, n_ent, rows, e0, cap = 2 * k, 300, 70, 4, 130
    E, R, T = ref.entity_table("normal", n_ent, ki), ref.relation_table(ki), ref.triples(rows, n_ent)
    E[T[:5, 2]] = E[T[5, 2]]                  # ties among candidates
    Et = cu(E)
    Q, pos_int = D.eval_build_queries(L.ROTATE, Et, cu(R), ki, 1.0, cu(T), L.EVAL_O)
    slab = Et[e0:]
    S = D.eval_scores_dense(L.ROTATE, Q, slab, ki, 1.0).cpu().numpy()
    c, p = ref.cmp_int(-S), pos_int.cpu().numpy().astype(np.int64)
    rs = np.random.RandomState(k)
    sizes = [0, cap, 1, 64, 65, 0, 17, cap]   # 8 segments = two groups of four
    pairs = np.zeros((len(sizes), cap), np.int64)
    want = np.zeros((2, rows), np.int64)
    for sgm, n in enumerate(sizes):
        r, e = rs.randint(0, rows, n), rs.randint(0, n_ent - e0, n)
        pairs[sgm, :n] = (r.astype(np.int64) << 32) | (e + e0)
        pairs[sgm, n:] = (1 << 40) | 0x7fffffff      # never read
        np.add.at(want[0], r, c[r, e] > p[r])
        np.add.at(want[1], r, c[r, e] == p[r])
    pcount = np.array(sizes + [0], np.int32)
    cnt = torch.zeros((2, rows), dtype=torch.int32, device="cuda")
    D.eval_rescore_pairs(L.ROTATE, Q, pos_int, slab, e0, ki, 1.0, cu(pairs.reshape(-1)), cu(pcount), len(sizes), cnt[0], cnt[1], 4)
    assert np.array_equal(cnt.cpu().numpy(), want)
    # a non-linear link with RotatE: refused
    with pytest.raises(L.EmgError, match="linear link"):
        D.eval_rescore_pairs(L.ROTATE, Q, pos_int, slab, e0, ki, 1.0, cu(pairs.reshape(-1)), cu(pcount), len(sizes), cnt[0], cnt[1], 4,
                             link=L.LINK_TANH)
    # and the exact count keeps refusing a precision
    with pytest.raises(L.EmgError):
        D.eval_count(L.ROTATE, Q, pos_int, slab, ki, 1.0, cnt[0], cnt[1], precision=2)
