"""Kernels on tables past 4 GiB and past 2^23 rows (helper and layout: tests/_large_tables.py; the conditions on these inputs:
tests/test_large_tables_host.py).

Every case makes two assertions.  (a) BIT EQUALITY with the compact twin: the same rows in an ordinary table, the same call —
address arithmetic must not change a value.  (b) agreement with a plain float64 / exact-integer reference on the gathered
rows, at the tolerance of the family's small-shape test, which is named beside the assert.  After every sparse-giant case the
arena's non-NaN cells are counted: a store through a cut offset lands on a NaN cell and changes the count.

SPARSE-GIANT cases read and write tables whose rows lie 2 097 168 bytes apart (16.02 GiB for 8200 rows; 8.02 GiB for 4104
where less memory is free); MANY-NARROW cases use 2^24 + 2^23 + 5 rows of 16 bytes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import c_oracle as co  # noqa: E402
from oracle import emgraph_oracle as orc  # noqa: E402
from tests import _large_tables as lt  # noqa: E402
from tests import _rotate_ref as rotref  # noqa: E402
from tests import _simple_ref as simref  # noqa: E402
from tests.test_hip_kernels import score_tol  # noqa: E402

F32 = np.float32
MID = orc.MODEL_IDS
BASE_MODELS = ["TransE_L1", "TransE_L2", "DistMult", "ComplEx", "HolE"]


def libs():
    from emgraph_amd import _lib as L
    from emgraph_amd import device as D
    D.require_gpu()
    return L, D


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def eq_bits(a, b, what=""):
    np.testing.assert_array_equal(lt.bits(a), lt.bits(b), err_msg=what)


_ARENAS = []          # the module's arena while it lives: the many-narrow cases release its memory before they allocate theirs


@pytest.fixture(scope="module")
def arena():
    libs()
    free = torch.cuda.mem_get_info()[0]
    n_rows = lt.choose_span(free)
    if n_rows is None:
        pytest.skip("the sparse-giant arena needs %d bytes free twice over, the device has %d free" % (lt.arena_bytes(lt.SPAN_SMALL), free))
    a = lt.Arena(n_rows)
    _ARENAS.append(a)
    print("\nsparse-giant span: %d rows, %.2f GiB" % (n_rows, lt.arena_bytes(n_rows) / 2.0**30))
    yield a
    a.free()
    _ARENAS.clear()


@pytest.fixture()
def giant(arena):
    """the arena, all NaN, for one case; checked for stray stores when the case ends"""
    arena.reset()
    yield arena
    torch.cuda.synchronize()
    arena.check_no_stray_write()


def test_the_span_in_use_is_the_largest_the_device_holds(arena, record_property):
    """The arena takes the 16.02 GiB span (8200 rows: past byte 2^34 and element 2^32) wherever twice its size is free, the
    8.02 GiB span only on a smaller device; which one ran is recorded with the test and printed by the fixture."""
    arena.reset()
    free_now = torch.cuda.mem_get_info()[0] + lt.arena_bytes(arena.n_rows)
    assert arena.n_rows == lt.choose_span(free_now)
    assert (arena.n_rows == lt.SPAN_LARGE) == (free_now >= 2 * lt.arena_bytes(lt.SPAN_LARGE))
    record_property("sparse_giant_rows", arena.n_rows)
    assert arena.buf.numel() == lt.arena_floats(arena.n_rows)
    assert arena.count_written() == 0


# ================================================================ sparse-giant: scoring
# name -> (model id, oracle name, k, k_int, scale)
def score_models():
    from emgraph_amd import _lib as L
    k = 25
    return {"TransE_L1": (L.TRANSE_L1, "TransE_L1", 50, 50, 1.0), "TransE_L2": (L.TRANSE_L2, "TransE_L2", 50, 50, 1.0),
            "DistMult": (L.DISTMULT, "DistMult", 50, 50, 1.0), "ComplEx": (L.COMPLEX, "ComplEx", k, 2 * k, 1.0),
            "HolE": (L.HOLE, "HolE", k, 2 * k, float(F32(2 / k))), "TransE_P": (L.TRANSE_P, "TransE_P:3.0", 50, 50, 3.0),
            "RotatE": (L.ROTATE, None, k, 2 * k, 1.0), "SimplE": (L.SIMPLE, None, k, 2 * k, simref.SCALE)}


def probe_triples(probes, seed):
    """every probe row as subject, as relation and as object in turn (three rotations of the probe list, then seeded ones)"""
    rs = np.random.RandomState(seed)
    n = len(probes)
    s = np.concatenate([probes, np.roll(probes, 1), np.roll(probes, 2), probes[rs.randint(0, n, n)]])
    p = np.concatenate([np.roll(probes, 2), probes, np.roll(probes, 1), probes[rs.randint(0, n, n)]])
    o = np.concatenate([np.roll(probes, 1), np.roll(probes, 2), probes, probes[rs.randint(0, n, n)]])
    return np.stack([s, p, o], 1).astype(np.int32)


def probe_tables(giant, name, ki, seed, model=None):
    """entity and relation tables holding the probe rows (arena views), their values, and the twins"""
    rs = np.random.RandomState(seed)
    n = len(giant.probes)
    E = (rs.randn(n, ki) * 0.3).astype(F32)
    R = (rs.randn(n, ki) * 0.3).astype(F32)
    if model == "RotatE":      # phases in the first half, the second half unused
        R[:, ki // 2:] = 0.0
        R[:, :ki // 2] = rs.uniform(-np.pi, np.pi, (n, ki // 2))
    Eb, Rb = giant.write("ent", giant.probes, E), giant.write("rel", giant.probes, R)
    return E, R, Eb, Rb, lt.compact(E), lt.compact(R)


@pytest.mark.parametrize("model", ["TransE_L1", "TransE_L2", "DistMult", "ComplEx", "HolE", "TransE_P", "RotatE", "SimplE"])
def test_giant_score_triples(giant, model):
    """emg_score_triples with subjects, relations and objects on both sides of every mark.  (b): score_tol of
    tests/test_hip_kernels.py::test_score_triples_vs_oracle for the five reference models; rtol 1e-4 / atol 1e-6 for TransE-p
    (test_transe_any_norm_forward_backward_vs_oracle) and RotatE (tests/test_rotate.py::test_scores_and_gradients_vs_float64);
    _simple_ref.score_bound for SimplE (tests/test_simple.py::test_scores_and_gradients_vs_float64)."""
    L, D = libs()
    mid, oname, k, ki, scale = score_models()[model]
    E, R, Eb, Rb, Es, Rs = probe_tables(giant, model, ki, seed=ki + mid, model=model)
    m = lt.Remap(giant.probes)
    X = probe_triples(giant.probes, seed=3)
    Xs = m.triples(X, rel=m)
    assert Eb.stride(0) == lt.LD and Eb.data_ptr() + 4 * lt.LD * int(X[:, 0].max()) - giant.buf.data_ptr() >= (1 << 33)
    big = D.score_triples(mid, Eb, Rb, ki, scale, cu(X))
    small = D.score_triples(mid, Es, Rs, ki, scale, cu(Xs))
    eq_bits(big, small, "strided table vs compact twin")
    got = big.cpu().numpy()
    assert np.all(np.isfinite(got))
    if model in BASE_MODELS:
        exp = orc.score_triples(oname, E, R, Xs, k=k)
        assert np.all(np.abs(got - exp) <= score_tol(oname, E, R, Xs, k)), np.abs(got - exp).max()
    elif model == "TransE_P":
        np.testing.assert_allclose(got, orc.score_triples(oname, E, R, Xs), rtol=1e-4, atol=1e-6)
    elif model == "RotatE":
        np.testing.assert_allclose(got, rotref.score_f64(E, R, Xs), rtol=1e-4, atol=1e-6)
    else:
        assert np.all(np.abs(got.astype(np.float64) - simref.score_f64(E, R, Xs)) <= simref.score_bound(E, R, Xs))


# ================================================================ sparse-giant: training pieces
@pytest.mark.parametrize("model", BASE_MODELS)
def test_giant_train_forward_and_backward(giant, model):
    """emg_train_forward / emg_train_backward: positives on the probe rows, negatives drawn from a pool of probe rows (the same
    Philox draws index the remapped pool of the twin).  (b): score_tol (test_train_forward_vs_oracle); gradient tables rtol
    1e-4, atol 1e-5 max|grad| (test_train_backward_vs_oracle)."""
    L, D = libs()
    mid, oname, k, ki, scale = score_models()[model]
    E, R, Eb, Rb, Es, Rs = probe_tables(giant, model, ki, seed=7 * ki + mid)
    m = lt.Remap(giant.probes)
    X = probe_triples(giant.probes, seed=5)
    Xs = m.triples(X, rel=m)
    B, eta, n = X.shape[0], 3, len(giant.probes)
    pool_b, pool_s = giant.probes.astype(np.int32), np.arange(n, dtype=np.int32)
    cb = D.corrupt_codes(B, eta, L.SIDE_SO, n, "cuda", entities_list=cu(pool_b), seed=9, counter=4)
    cs = D.corrupt_codes(B, eta, L.SIDE_SO, n, "cuda", entities_list=cu(pool_s), seed=9, counter=4)
    np.testing.assert_array_equal(m.codes(cb.cpu().numpy()), cs.cpu().numpy())
    ids = cb.cpu().numpy() & 0x7FFFFFFF
    assert ids.max() == giant.probes[-1] and set(ids.tolist()) == set(giant.probes.tolist())      # every probe row is a negative
    spb, snb = D.train_forward(mid, Eb, Rb, ki, scale, cu(X), eta, cb)
    sps, sns = D.train_forward(mid, Es, Rs, ki, scale, cu(Xs), eta, cs)
    eq_bits(spb, sps, "positive scores"); eq_bits(snb, sns, "negative scores")
    xneg = D.corrupt_expand(cu(Xs), eta, cs).cpu().numpy()
    assert np.all(np.abs(spb.cpu().numpy() - orc.score_triples(oname, E, R, Xs, k=k)) <= score_tol(oname, E, R, Xs, k))
    assert np.all(np.abs(snb.cpu().numpy() - orc.score_triples(oname, E, R, xneg, k=k)) <= score_tol(oname, E, R, xneg, k))
    # backward
    rs = np.random.RandomState(B)
    gpos, gneg = rs.randn(B).astype(F32), rs.randn(B * eta).astype(F32)
    ldc = lt.padded(ki)
    out = []
    for (Et, Rt, Xt, ct) in ((Eb, Rb, cu(X), cb), (Es, Rs, cu(Xs), cs)):
        ce = torch.zeros(((2 + eta) * B, ldc), dtype=torch.float32, device="cuda")
        cr = torch.zeros((B, ldc), dtype=torch.float32, device="cuda")
        de = torch.empty((2 + eta) * B, dtype=torch.int32, device="cuda")
        dr = torch.empty(B, dtype=torch.int32, device="cuda")
        D.train_backward(mid, Et, Rt, ki, scale, Xt, eta, ct, cu(gpos), cu(gneg), ce, cr, de, dr)
        out.append((ce, cr, de.cpu().numpy(), dr.cpu().numpy()))
    (ceb, crb, deb, drb), (ces, crs, des, drs) = out
    eq_bits(ceb, ces, "entity contributions"); eq_bits(crb, crs, "relation contributions")
    np.testing.assert_array_equal(m.to_small(deb), des)
    np.testing.assert_array_equal(m.to_small(drb), drs)
    np.testing.assert_array_equal(deb[:B], X[:, 0]); np.testing.assert_array_equal(deb[B:2 * B], X[:, 2])
    np.testing.assert_array_equal(deb[2 * B:], ids); np.testing.assert_array_equal(drb, X[:, 1])
    dE, dR = np.zeros((n, ki)), np.zeros((n, ki))
    np.add.at(dE, des, ces.cpu().numpy()[:, :ki].astype(np.float64))
    np.add.at(dR, drs, crs.cpu().numpy()[:, :ki].astype(np.float64))
    eE, eR = orc.score_grads(oname, E, R, Xs, gpos, k=k)
    a, b = orc.score_grads(oname, E, R, xneg, gneg, k=k)
    eE += a; eR += b
    np.testing.assert_allclose(dE, eE, rtol=1e-4, atol=1e-5 * max(np.abs(eE).max(), 1e-6))
    np.testing.assert_allclose(dR, eR, rtol=1e-4, atol=1e-5 * max(np.abs(eR).max(), 1e-6))


def test_giant_row_passes(giant):
    """emg_scatter_rows onto the probe rows, then emg_clip_rows, emg_lp_regularizer (with its in-place update) and
    emg_lp_grad_rows over EVERY row of the strided table.  (b): float64 — the scattered rows exactly; the clip and the
    regulariser's update at rtol 1e-5 (one multiply / a few operations per element in float32), its value at rtol 2e-5
    (test_loss_and_grads_vs_oracle's bar for a float64 accumulator)."""
    L, D = libs()
    k, n_rows = 50, giant.n_rows
    rs = np.random.RandomState(31)
    W = (rs.randn(n_rows, k) * 0.2).astype(F32)          # norms around 1.4: some rows above max_norm = 1.5, some below
    Wb, Ws = giant.write("ent", None, W), lt.compact(W)
    ids = giant.probes.astype(np.int32)[::-1].copy()     # distinct, not ascending
    rows = (rs.randn(len(ids), k) * 0.2).astype(F32)
    for t in (Wb, Ws):
        D.scatter_rows(t, k, lt.compact(rows), cu(ids))
    exp = W.copy(); exp[ids] = rows
    eq_bits(Wb, Ws, "scatter_rows")
    np.testing.assert_array_equal(Wb.cpu().numpy(), exp)
    for t in (Wb, Ws):
        D.clip_rows(t, k, 1.5)
    eq_bits(Wb, Ws, "clip_rows")
    nrm = np.sqrt((exp.astype(np.float64) ** 2).sum(1, keepdims=True))
    clipped = np.where(nrm > 1.5, exp * 1.5 / nrm, exp)
    assert (nrm > 1.5).sum() > 100 and (nrm < 1.5).sum() > 100
    np.testing.assert_allclose(Wb.cpu().numpy(), clipped, rtol=1e-5, atol=0)
    acc = [torch.zeros(1, dtype=torch.float64, device="cuda") for _ in range(2)]
    for t, a in zip((Wb, Ws), acc):
        D.lp_regularizer(t, k, 0.01, 3, 0.5, a)
    eq_bits(Wb, Ws, "lp_regularizer table")
    assert abs(acc[0].item() - acc[1].item()) <= 4096 * 2.0 ** -52 * abs(acc[0].item())      # (double atomics, one per workgroup: the order of the adds is free)
    c64 = clipped.astype(np.float64)
    np.testing.assert_allclose(acc[0].item(), 0.01 * (np.abs(c64) ** 3).sum(), rtol=2e-5)
    upd = c64 - 0.5 * 0.01 * 3 * c64 * np.abs(c64)
    np.testing.assert_allclose(Wb.cpu().numpy(), upd, rtol=1e-5, atol=1e-9)
    out = []
    for t in (Wb, Ws):
        contrib = torch.zeros((n_rows, lt.padded(k)), dtype=torch.float32, device="cuda")
        dest = torch.empty(n_rows, dtype=torch.int32, device="cuda")
        a = torch.zeros(1, dtype=torch.float64, device="cuda")
        D.lp_grad_rows(t, k, 0.01, 2, contrib, dest, a)
        out.append((contrib, dest, a.item()))
    eq_bits(out[0][0], out[1][0], "lp_grad_rows")
    assert abs(out[0][2] - out[1][2]) <= 4096 * 2.0 ** -52 * abs(out[0][2])
    np.testing.assert_array_equal(out[0][1].cpu().numpy(), np.arange(n_rows))
    np.testing.assert_allclose(out[0][0].cpu().numpy()[:, :k], 0.01 * 2 * Wb.cpu().numpy().astype(np.float64), rtol=1e-6)


def test_giant_init_table(giant):
    """emg_init_table counts by (row, column) — element (r, c) takes Philox counter (r * k_int + c) / 4 (include/emgraph_hip.h),
    not by the flat offset r * ld + c: the strided table and the compact one hold the same bits, and the padding stays
    untouched.  (b): the distribution's bounds and moments (test_device_initialisers_distribution_and_determinism)."""
    L, D = libs()
    k, n_rows = 50, giant.n_rows
    Wb = giant.table("ent", k)
    from emgraph_amd.training import alloc_table
    Ws = alloc_table(n_rows, k, torch.device("cuda"))
    for t in (Wb, Ws):
        D.init_table(t, k, "uniform", -0.25, 0.75, 11, 1)
    giant.owned += n_rows * k                            # (k of the padded 52 columns: the pad is not the entry's)
    eq_bits(Wb, Ws, "init_table")
    u = Wb.cpu().numpy().astype(np.float64)
    assert u.min() >= -0.25 and u.max() < 0.75
    assert abs(u.mean() - 0.25) < 2e-3 and abs(u.var() - 1.0 / 12) < 2e-3


# ================================================================ sparse-giant: optimizer
@pytest.mark.parametrize("opt", ["sgd", "momentum", "adagrad", "adam", "adam_lazy"])
def test_giant_apply_rows(giant, opt):
    """emg_apply_rows with the table and its states as arena views: destinations on the probe rows, each mark row with a
    segment of its own, two of them longer than 64 contributions (block tasks: apply_long_kernel) on rows past byte 2^33 and
    2^34.  Dense-equivalent Adam walks every row of the three tables, so there every row is initialised.  (b): one step of
    tests/test_hip_kernels.py::test_apply_rows_vs_oracle, rtol 2e-5 / atol 2e-6; for SGD also the exact sums of
    test_counting_grouping_edge_shapes."""
    L, D = libs()
    k, n_rows = 72, giant.n_rows
    dense = opt == "adam"
    kept = np.arange(n_rows, dtype=np.int64) if dense else giant.probes
    m = lt.Remap(kept)
    rs = np.random.RandomState(8 + len(opt))
    n = len(kept)
    W = rs.randn(n, k).astype(F32)
    rows = None if dense else kept
    Wb, Ws = giant.write("ent", rows, W), lt.compact(W)
    st_b, st_s = [None, None], [None, None]
    init = {"momentum": [0.0], "adagrad": [0.1], "adam": [0.0, 0.0], "adam_lazy": [0.0, 0.0]}.get(opt, [])
    for j, v in enumerate(init):
        S = np.full((n, k), v, F32)
        st_b[j], st_s[j] = giant.write("ent_s%d" % j, rows, S), lt.compact(S)
    long_rows = [r for r in (giant.n_rows - 1, 4096) if r < giant.n_rows]
    dest = np.concatenate([giant.probes[rs.randint(0, len(giant.probes), 900)], giant.probes, np.repeat(long_rows, [200, 131])]).astype(np.int32)
    rs.shuffle(dest)
    n_c = len(dest)
    contrib = rs.randn(n_c, k).astype(F32)
    lr, mu, b1, b2, eps = 0.05, 0.9, 0.9, 0.999, 1e-7
    lr_t = lr * np.sqrt(1 - b2) / (1 - b1)
    for (Wt, st, dd, nr) in ((Wb, st_b, dest, n_rows), (Ws, st_s, m.to_small(dest), n)):
        tag = torch.zeros(nr, dtype=torch.int32, device="cuda")
        ws = torch.zeros(D.apply_workspace_bytes(n_c, nr, k), dtype=torch.uint8, device="cuda")
        D.apply_rows(L.OPT_IDS[opt], Wt, k, st[0], st[1], tag, 1, cu(contrib), cu(dd), n_c, (lr, mu, b1, b2, eps, lr_t), ws)
    torch.cuda.synchronize()
    sel = cu(kept)
    eq_bits(Wb[sel], Ws, "table")
    for j in range(len(init)):
        eq_bits(st_b[j][sel], st_s[j], "state %d" % j)
    # (b)
    got = Ws.cpu().numpy()
    ds = m.to_small(dest)
    G = np.zeros((n, k), np.float64)
    np.add.at(G, ds, contrib.astype(np.float64))
    touched = np.zeros(n, bool); touched[ds] = True
    if opt == "adam_lazy":
        g = G.astype(F32)
        mm = F32(1 - b1) * g; vv = F32(1 - b2) * g ** 2
        exp = W.copy()
        exp[touched] = W[touched] - F32(lr_t) * mm[touched] / (np.sqrt(vv[touched]) + F32(eps))
    else:
        exp = orc.opt_apply(opt, W.copy(), G, orc.opt_init(opt, W.shape), lr=lr, momentum=mu, beta1=b1, beta2=b2, eps=eps,
                            touched=None if opt == "adam" else touched)
    np.testing.assert_allclose(got, exp, rtol=2e-5, atol=2e-6)
    if opt != "adam":
        np.testing.assert_array_equal(got[~touched], W[~touched])
    if opt == "sgd":
        order, nv = lt.stable_order(ds, n)
        sums = lt.segment_sums_f32(contrib, ds, order, block=64)
        exact = W.copy()
        for r, g in sums.items():
            exact[r] = exact[r] - F32(lr) * g
        np.testing.assert_array_equal(got, exact)


@pytest.mark.parametrize("model", ["TransE_L1", "ComplEx"])
def test_giant_shared_relneg_and_batchreg(giant, model):
    """emg_shared_forward / _backward (chunks of 8 positives against common draws), emg_relneg_forward / _backward (the relation
    replaced by probe rows of the strided relation table) and emg_batchreg on the strided tables; every row is initialised and
    the twin keeps the identical ids.  (a) scores, contribution rows and destinations to the bit, the regulariser's value to the order of its atomic adds.
    (b) tests/_shared_ref.py and tests/_relneg_ref.py: the float64 gradient tables at the bars of test_shared_negatives /
    test_train_backward_vs_oracle; tests/_batchreg_ref.py: rows and destinations to the bit, the value at rtol 1e-12
    (tests/test_batch_regularizer.py)."""
    L, D = libs()
    mid, oname, k, ki, scale = score_models()[model]
    E, R, Eb, Rb, Es, Rs = dense_tables(giant, ki, seed=ki + 17 * mid, plant=False)
    p = giant.probes
    X = probe_triples(p, seed=43)
    B, Cc, eta, n_rel = X.shape[0], 8, 6, giant.n_rows
    G = -(-B // Cc)
    rs = np.random.RandomState(B + 2)
    chunk_codes = D.corrupt_codes(G, eta, L.SIDE_SO, len(p), "cuda", entities_list=cu(p.astype(np.int32)), seed=7, counter=1)
    q = p[rs.randint(0, len(p), (eta, B))]                               # replacement relations: probe rows other than the positive's
    q = np.where(q == X[None, :, 1], p[(np.searchsorted(p, q) + 1) % len(p)], q)
    rel_codes = (q - (q > X[None, :, 1])).reshape(-1).astype(np.int32)   # p' = idx + (idx >= p)
    assert rel_codes.min() >= 0 and rel_codes.max() < n_rel - 1
    gpos, gneg = rs.randn(B).astype(F32), rs.randn(B * eta).astype(F32)
    ldc = lt.padded(ki)
    res = []
    for (Et, Rt) in ((Eb, Rb), (Es, Rs)):
        Xt, z = cu(X), lambda n, dt=torch.float32: torch.zeros(n, dtype=dt, device="cuda")  # noqa: E731
        sp, sn = D.shared_forward(mid, Et, Rt, ki, scale, Xt, Cc, eta, chunk_codes)
        ce, cr = z((2 * B + eta * G, ldc)), z((B, ldc))
        de, dr = z(2 * B + eta * G, torch.int32), z(B, torch.int32)
        D.shared_backward(mid, Et, Rt, ki, scale, Xt, Cc, eta, chunk_codes, cu(gpos), cu(gneg), ce, cr, de, dr, raw_pos=sp, raw_neg=sn)
        rp, rn = D.relneg_forward(mid, Et, Rt, ki, scale, Xt, eta, cu(rel_codes))
        ce2, cr2 = z((2 * B, ldc)), z((B + eta * B, ldc))
        de2, dr2 = z(2 * B, torch.int32), z(B + eta * B, torch.int32)
        D.relneg_backward(mid, Et, Rt, ki, scale, Xt, eta, cu(rel_codes), cu(gpos), cu(gneg), ce2, cr2, de2, dr2, raw_pos=rp, raw_neg=rn)
        ce3, cr3, de3, dr3 = z((2 * B, ldc)), z((B, ldc)), z(2 * B, torch.int32), z(B, torch.int32)
        val = z(1, torch.float64)
        D.batch_reg(Et, Rt, ki, Xt, 3, 1e-2, 5e-3, L.BATCHREG_PLAIN, L.BATCHREG_PLAIN, ce3, de3, cr3, dr3, val)
        res.append([sp, sn, ce, cr, de, dr, rp, rn, ce2, cr2, de2, dr2, ce3, cr3, de3, dr3, val])
    for a, b in zip(res[0][:16], res[1][:16]):
        eq_bits(a, b)
    # the value: every workgroup adds its (positive) partial sum to the device double with one atomic, in no fixed order — two
    # runs differ by at most (workgroups - 1) 2^-52 relative; fewer than 4096 workgroups here
    assert abs(res[0][16].item() - res[1][16].item()) <= 4096 * 2.0 ** -52 * res[0][16].item()
    sp, sn, ce, cr, de, dr, rp, rn, ce2, cr2, de2, dr2 = res[0][:12]
    assert np.all(np.isfinite(sn.cpu().numpy())) and np.all(np.isfinite(rn.cpu().numpy())) and float(ce.abs().max()) > 0
    np.testing.assert_array_equal(dr2.cpu().numpy()[B:], q.reshape(-1))        # the replaced relations are the probe rows
    np.testing.assert_array_equal(de.cpu().numpy()[:B], X[:, 0])
    assert set(de.cpu().numpy()[2 * B:].tolist()) <= set(p.tolist()) and float(res[0][16].item()) > 0
    # (b) the families' own references
    from tests import _batchreg_ref as brref
    from tests import _relneg_ref as rnref
    from tests import _shared_ref as shref
    n = giant.n_rows
    cc = chunk_codes.cpu().numpy()
    np.testing.assert_array_equal(de.cpu().numpy()[2 * B:], shref.split_codes(cc)[0])
    want_E, want_R = shref.dense_grads(mid, E, R, X, shref.expand_codes(cc, B, Cc, eta), eta, gpos, gneg, scale)
    for got, dest, want in ((ce, de, want_E), (cr, dr, want_R)):
        new = shref.scatter_rows(got.cpu().numpy()[:, :ki], dest.cpu().numpy(), n)
        # tests/test_shared_negatives.py: at most 4 x the ordinary backward's error, itself at most 1e-4 max(1, max|g|)
        assert np.abs(new - want).max() <= 4e-4 * max(1.0, np.abs(want).max())
    trip = np.concatenate([X.astype(np.int64), rnref.negatives(X, rel_codes)])
    np.testing.assert_array_equal(trip[B:, 1], q.reshape(-1))
    dE, dR = rnref.dense_grads(mid, E, R, trip, np.concatenate([gpos, gneg]), scale)[:2]
    for got, dest, want in ((ce2, de2, dE), (cr2, dr2, dR)):
        new = shref.scatter_rows(got.cpu().numpy()[:, :ki], dest.cpu().numpy(), n)
        np.testing.assert_allclose(new, want, rtol=1e-4, atol=1e-5 * max(np.abs(want).max(), 1e-6))     # test_train_backward_vs_oracle
    ge, wde, gr, wdr, wval = brref.batch_reg(E, R, X, 3, 1e-2, 5e-3, False, False)      # tests/test_batch_regularizer.py: to the bit
    eq_bits(res[0][12][:, :ki], ge); eq_bits(res[0][13][:, :ki], gr)
    np.testing.assert_array_equal(res[0][14].cpu().numpy(), wde); np.testing.assert_array_equal(res[0][15].cpu().numpy(), wdr)
    np.testing.assert_allclose(res[0][16].item(), wval, rtol=1e-12)


def opt_tables(giant, opt, ki, seed, scale=0.3, kept=None):
    """entity and relation tables with their optimizer states as arena views, and the twins: the probe rows — every row for the
    dense-equivalent Adam, whose dense pass walks the tables and both moments.  Returns (kept rows, host E, host R, big, small)
    with big / small = dict(ent, rel, states = [ent0, ent1, rel0, rel1])."""
    dense = opt == "adam"
    if kept is None or dense:
        kept = np.arange(giant.n_rows, dtype=np.int64) if dense else giant.probes
    rows = None if dense else kept
    rs = np.random.RandomState(seed)
    n = len(kept)
    E, R = (rs.randn(n, ki) * scale).astype(F32), (rs.randn(n, ki) * scale).astype(F32)
    big = {"ent": giant.write("ent", rows, E), "rel": giant.write("rel", rows, R), "states": [None] * 4}
    small = {"ent": lt.compact(E), "rel": lt.compact(R), "states": [None] * 4}
    init = {"momentum": [0.0], "adagrad": [0.1], "adam": [0.0, 0.0], "adam_lazy": [0.0, 0.0]}.get(opt, [])
    for t, tab in enumerate(("ent", "rel")):
        for j, v in enumerate(init):
            S = np.full((n, ki), v, F32)
            big["states"][2 * t + j] = giant.write("%s_s%d" % (tab, j), rows, S)
            small["states"][2 * t + j] = lt.compact(S)
    return kept, E, R, big, small


def same_tables(kept, big, small):
    sel = cu(kept)
    eq_bits(big["ent"][sel], small["ent"], "entity table")
    eq_bits(big["rel"][sel], small["rel"], "relation table")
    for j in range(4):
        if big["states"][j] is not None:
            eq_bits(big["states"][j][sel], small["states"][j], "state %d" % j)


@pytest.mark.parametrize("opt", ["sgd", "momentum", "adagrad", "adam", "adam_lazy"])
def test_giant_prepare_batch_and_apply_grouped(giant, opt):
    """emg_prepare_batch + emg_apply_grouped on both tables, the four state tables arena views too (the relation states at
    columns 8192 and 10240): negatives from a pool of probe rows, a hub subject and a hub relation on rows past byte 2^33 (block
    tasks).  Both sides group with the counting form (tables below 131072 rows).  (b) SGD: the exact sums of
    test_counting_grouping_edge_shapes on both tables; the other optimizers' arithmetic has its (b) in test_giant_apply_rows."""
    L, D = libs()
    k = 72
    kept, E, R, big, small = opt_tables(giant, opt, k, seed=40 + len(opt), scale=1.0)
    m = lt.Remap(kept)
    X = probe_triples(giant.probes, seed=6)
    hub = int(giant.probes[-1])
    X = np.concatenate([X, np.stack([np.full(150, hub), np.full(150, 4096), giant.probes[np.arange(150) % len(giant.probes)]], 1).astype(np.int32)])
    B, eta, sides = X.shape[0], 4, (L.SIDE_SO,)
    rs = np.random.RandomState(B)
    n_ce = (2 + eta) * B
    ce, cr = rs.randn(n_ce, k).astype(F32), rs.randn(B, k).astype(F32)
    lr, mu, b1, b2, eps = 0.05, 0.9, 0.9, 0.999, 1e-7
    hyper = (lr, mu, b1, b2, eps, lr * np.sqrt(1 - b2) / (1 - b1))
    dests = []
    for (T, Xt, pool, nr) in ((big, X, giant.probes.astype(np.int32), giant.n_rows),
                              (small, m.triples(X, rel=m), m.to_small(giant.probes).astype(np.int32), len(kept))):
        codes, de, dr, we, wr, _, _ = prepare(D, Xt, eta, sides, pool, nr, nr, k, False)
        for (tab, j0, contrib, nc, ws_) in (("ent", 0, ce, n_ce, we), ("rel", 2, cr, B, wr)):
            tag = torch.zeros(nr, dtype=torch.int32, device="cuda")
            D.apply_grouped(L.OPT_IDS[opt], T[tab], k, T["states"][j0], T["states"][j0 + 1], tag, 1, cu(contrib), nc, 0, hyper, ws_)
        dests.append((de.cpu().numpy(), dr.cpu().numpy()))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(m.to_small(dests[0][0]), dests[1][0]); np.testing.assert_array_equal(m.to_small(dests[0][1]), dests[1][1])
    same_tables(kept, big, small)
    if opt == "sgd":
        for (W0, got, dest, contrib) in ((E, small["ent"], dests[1][0], ce), (R, small["rel"], dests[1][1], cr)):
            order, nv = lt.stable_order(dest, len(kept))
            exact = W0.copy()
            for r, g in lt.segment_sums_f32(contrib, dest, order, block=64).items():
                exact[r] = exact[r] - F32(lr) * g
            np.testing.assert_array_equal(got.cpu().numpy(), exact)
            assert np.bincount(dest).max() > 64


@pytest.mark.parametrize("opt,policy", [("sgd", "0"), ("sgd", "1"), ("momentum", "0"), ("adagrad", "0"), ("adam", "0"), ("adam_lazy", "0")])
def test_giant_train_step(giant, monkeypatch, opt, policy):
    """emg_train_step (the one-call step of the C ABI) with injected draws, tables and states arena views.  The cache-policy form
    of the fused SGD kernel is chosen from the table's byte size (n_ent x row stride against the 256 MB of Infinity Cache), which
    the strided table changes: EMG_CACHE_POLICY pins the same form on both sides, and the library's count of cache-policy
    launches shows that the forced form ran on the strided table.  (a) tables and states to the bit, loss_accum to the order of its atomic adds.  (b) SGD: the
    oracle's gradients through one step at the tolerance of test_wide_rows_train_in_column_blocks (rtol 2e-4, atol 2e-5 lr
    max|grad|); the loss at 1e-4 relative, the scores' bar (test_score_triples_vs_oracle)."""
    L, D = libs()
    monkeypatch.setenv("EMG_CACHE_POLICY", policy)
    lib = L.load()
    k, ki = 24, 48
    kept, E, R, big, small = opt_tables(giant, opt, ki, seed=50 + len(opt), scale=0.2)
    m = lt.Remap(kept)
    X = probe_triples(giant.probes, seed=8)
    B, eta = X.shape[0], 3
    rs = np.random.RandomState(B + 1)
    repl = giant.probes[rs.randint(0, len(giant.probes), B * eta)].astype(np.int32)
    mask = rs.randint(0, 2, B * eta).astype(np.int32)
    lr, mu, b1, b2, eps = 0.05, 0.9, 0.9, 0.999, 1e-7
    hyper = (lr, mu, b1, b2, eps, lr * np.sqrt(1 - b2) / (1 - b1))
    losses, ran = [], []
    for (T, Xt, rp, nr) in ((big, X, repl, giant.n_rows), (small, m.triples(X, rel=m), m.to_small(repl), len(kept))):
        acc = torch.zeros(1, dtype=torch.float64, device="cuda")
        ws = torch.zeros(D.train_step_workspace_bytes(B, eta, ki, nr, nr), dtype=torch.uint8, device="cuda")
        tags = (torch.zeros(nr, dtype=torch.int32, device="cuda"), torch.zeros(nr, dtype=torch.int32, device="cuda"))
        before = lib.emg_cache_policy_launches()
        D.train_step(L.COMPLEX, T["ent"], T["rel"], ki, 1.0, cu(Xt), eta, [L.SIDE_SO], L.LOSS_IDS["nll"], acc, L.OPT_IDS[opt], 1, hyper, ws,
                     states=tuple(T["states"]), tags=tags, n_choices=nr, inj_mask=cu(mask), inj_repl=cu(rp), inplace=True)
        torch.cuda.synchronize()
        ran.append(lib.emg_cache_policy_launches() - before)
        losses.append(acc.item())
    assert (ran[0] > 0) == (policy == "1") and (ran[1] > 0) == (policy == "1"), (policy, ran)
    same_tables(kept, big, small)
    # (the loss: positive terms added to a device double with one atomic per workgroup, in no fixed order)
    assert abs(losses[0] - losses[1]) <= 4096 * 2.0 ** -52 * losses[0]
    Xs = m.triples(X, rel=m)
    codes = D.corrupt_codes(B, eta, L.SIDE_SO, len(kept), "cuda", inj_mask=cu(mask), inj_repl=cu(m.to_small(repl)))
    xneg = D.corrupt_expand(cu(Xs), eta, codes).cpu().numpy()
    sp, sn = orc.score_triples("ComplEx", E, R, Xs, k=k), orc.score_triples("ComplEx", E, R, xneg, k=k)
    np.testing.assert_allclose(losses[0], float(orc.loss_apply("nll", np.tile(sp, eta) if orc.REQUIRE_SAME_SIZE["nll"] else sp, sn, eta, {})), rtol=1e-4)
    if opt == "sgd":
        dE, dR = orc.train_grads("ComplEx", E, R, Xs, eta, "nll", None, [xneg], k=k)
        np.testing.assert_allclose(small["ent"].cpu().numpy(), E - lr * dE, rtol=2e-4, atol=2e-5 * max(np.abs(dE).max(), 1e-6) * lr + 1e-7)
        np.testing.assert_allclose(small["rel"].cpu().numpy(), R - lr * dR, rtol=2e-4, atol=2e-5 * max(np.abs(dR).max(), 1e-6) * lr + 1e-7)
        assert np.abs(small["ent"].cpu().numpy() - E).max() > 0.5 * lr * np.abs(dE).max()


def test_giant_deferred_catchup_and_materialize(giant):
    """Keras Adam with its dense pass DEFERRED, table and both moments arena views: every row was last written at step 1 (tag = 1;
    a tag of 0 means "never written": zero moments, which a zero gradient does not move), three steps pass in which nothing touches
    the table, then emg_deferred_catchup replays them for the destinations of a grouping (probe rows, two
    segments longer than 64 on rows past byte 2^33), emg_apply_grouped_ex(deferred_dense = 1) applies step 5 to them, and
    emg_deferred_materialize brings every other row of the 8200 to step 5.  (a) table, moments and tags to the bit.  (b) steps 2 .. 5
    of the oracle's dense-equivalent Adam (zero gradient in the first three), rtol 2e-5 / atol 2e-6
    (test_apply_rows_vs_oracle)."""
    import ctypes as C
    L, D = libs()
    lib = L.load()
    k, n, steps = 72, giant.n_rows, 5
    rs = np.random.RandomState(71)
    W = rs.randn(n, k).astype(F32)
    M = (rs.randn(n, k) * 0.1).astype(F32)
    V = (rs.rand(n, k) * 0.01 + 1e-4).astype(F32)
    lr, mu, b1, b2, eps = 0.05, 0.9, 0.9, 0.999, 1e-7
    lr_t = [0.0] + [lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t) for t in range(1, steps + 1)]
    hist = cu(np.array(lr_t, F32))
    p = giant.probes
    dest = np.concatenate([p[rs.randint(0, len(p), 600)], p, np.repeat([n - 1, 4096], [150, 90])]).astype(np.int32)
    rs.shuffle(dest)
    n_c = len(dest)
    contrib = cu(rs.randn(n_c, k).astype(F32))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    sides = []
    for big in (True, False):
        if big:
            Wt, Mt, Vt = giant.write("ent", None, W), giant.write("ent_s0", None, M), giant.write("ent_s1", None, V)
        else:
            Wt, Mt, Vt = lt.compact(W), lt.compact(M), lt.compact(V)
        tag = torch.ones(n, dtype=torch.int32, device="cuda")
        ws = torch.zeros(D.apply_workspace_bytes(n_c, n, k), dtype=torch.uint8, device="cuda")
        D.group_dest(cu(dest), n_c, n, ws)
        h = D._hyper8((lr, mu, b1, b2, eps, lr_t[steps]))
        L.check(lib.emg_deferred_catchup(L.OPT_ADAM, Wt.data_ptr(), n, Wt.stride(0), k, Mt.data_ptr(), Vt.data_ptr(), tag.data_ptr(), h,
                                         hist.data_ptr(), steps - 1, None, ws.data_ptr(), ws.numel(), n_c, 0, -1, stream), "emg_deferred_catchup")
        a = D._apply_args(L.OPT_ADAM, Wt, k, Mt, Vt, tag, steps, contrib, n_c, 0, (lr, mu, b1, b2, eps, lr_t[steps]), ws)
        a.deferred_dense = 1
        L.check(lib.emg_apply_grouped_ex(C.byref(a), stream), "emg_apply_grouped_ex")
        torch.cuda.synchronize()
        tag_mid = tag.cpu().numpy().copy()
        L.check(lib.emg_deferred_materialize(L.OPT_ADAM, Wt.data_ptr(), n, Wt.stride(0), k, Mt.data_ptr(), Vt.data_ptr(), tag.data_ptr(), h,
                                             hist.data_ptr(), steps, None, stream), "emg_deferred_materialize")
        torch.cuda.synchronize()
        sides.append((Wt, Mt, Vt, tag.cpu().numpy(), tag_mid))
    for a_, b_ in zip(sides[0][:3], sides[1][:3]):
        eq_bits(a_, b_)
    np.testing.assert_array_equal(sides[0][3], sides[1][3]); np.testing.assert_array_equal(sides[0][4], sides[1][4])
    touched = np.zeros(n, bool); touched[dest] = True
    assert np.all(sides[0][4][touched] == steps) and np.all(sides[0][4][~touched] == 1)     # before materialize: only the batch's rows moved
    assert np.all(sides[0][3] == steps)
    st = orc.opt_init("adam", W.shape)
    st["m"], st["v"], st["t"] = M.copy(), V.copy(), 1
    G = np.zeros((n, k), np.float64)
    np.add.at(G, dest, contrib.cpu().numpy().astype(np.float64))
    exp = W.copy()
    for t in range(2, steps + 1):
        exp = orc.opt_apply("adam", exp, G if t == steps else np.zeros_like(G), st, lr=lr, momentum=mu, beta1=b1, beta2=b2, eps=eps, touched=None)
    np.testing.assert_allclose(sides[1][0].cpu().numpy(), exp, rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(sides[1][1].cpu().numpy(), st["m"], rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(sides[1][2].cpu().numpy(), st["v"], rtol=2e-5, atol=2e-8)


# name -> (model, optimizer, fused loss or None = external dL/dscore, in place, state window, expected in-place form, cache policy)
BACKWARD_EX = {
    "sgd_pairwise_inplace": ("TransE_L1", "sgd", "pairwise", True, 0, 1, "0"),
    "sgd_nll_factored_inplace": ("DistMult", "sgd", "nll", True, 0, 1, "0"),
    "sgd_nll_cache_policy": ("ComplEx", "sgd", "nll", True, 0, 1, "1"),
    "adagrad_abs_margin_chunkwise": ("ComplEx", "adagrad", "absolute_margin", True, 0, 2, "0"),
    "adagrad_nll_window": ("ComplEx", "adagrad", "nll", True, 1, 4, "0"),
    "adam_lazy_nll_window": ("DistMult", "adam_lazy", "nll", True, 1, 5, "0"),
    "momentum_nll_through_the_apply": ("ComplEx", "momentum", "nll", False, 0, 0, "0"),
    "external_gradient": ("TransE_L2", "sgd", None, False, 0, 0, "0"),
}


@pytest.mark.parametrize("case", sorted(BACKWARD_EX))
def test_giant_train_backward_ex(giant, monkeypatch, case):
    """emg_prepare_batch + emg_train_backward_ex + emg_apply_grouped as emg_train_step chains them, with the forms the one-call
    step does not choose from Python: every fused loss (pairwise, NLL, absolute margin) and the external-gradient pass, factored
    and full contribution rows, singletons updated IN PLACE by SGD (form 1, also in the cache-policy form), by a stateful
    optimizer chunk by chunk (form 2) and through the state window with one / two state rows (forms 4 / 5), and everything
    through the apply (form 0).  WHICH FORM RAN: emg_train_backward_form on the very argument record of each call — the same on
    both sides, and the one the case names.  (The riders of a fused launch are attached only by a plan that has later batches
    to prepare: they are not an argument of this entry.)  (a) tables, states, raw scores to the bit; the loss to the order of
    its atomic adds.  (b) the loss at 1e-4 relative and the raw scores at score_tol (test_train_forward_vs_oracle); SGD with
    NLL: the oracle's gradients through the step, rtol 2e-4, atol 2e-5 lr max|grad| (test_wide_rows_train_in_column_blocks);
    the external pass: test_train_backward_vs_oracle's rtol 1e-4, atol 1e-5 max|grad| on the update."""
    import ctypes as C
    L, D = libs()
    model, opt, loss, inplace, window, want_ip, policy = BACKWARD_EX[case]
    monkeypatch.setenv("EMG_CACHE_POLICY", policy)
    lib = L.load()
    seen = []

    class Args(L.BackwardArgs):        # the wrapper's argument record, with the state window set and kept for the form query
        def __init__(self):
            super().__init__()
            self.inplace_window = window
            seen.append(self)
    monkeypatch.setattr(L, "BackwardArgs", Args)
    mid, oname = MID[model], model
    k = 24
    ki = 2 * k if model in ("ComplEx", "HolE") else 48
    kk = k if model in ("ComplEx", "HolE") else 48
    # negatives from a pool of the probe rows and 2500 seeded rows more: most of them are drawn once (singletons: the in-place forms)
    kept = np.union1d(giant.probes, np.random.RandomState(12).randint(0, giant.n_rows, 2500))
    kept, E, R, big, small = opt_tables(giant, opt, ki, seed=60 + len(case), scale=0.2, kept=kept)
    m = lt.Remap(kept)
    X = probe_triples(giant.probes, seed=10)
    B, eta = X.shape[0], 3
    n_ce = (2 + eta) * B
    factored = model not in ("TransE_L1", "TransE_L2")
    rs = np.random.RandomState(B + 3)
    gpos, gneg = rs.randn(B).astype(F32), rs.randn(B * eta).astype(F32)
    lr, mu, b1, b2, eps = 0.05, 0.9, 0.9, 0.999, 1e-7
    hyper = (lr, mu, b1, b2, eps, lr * np.sqrt(1 - b2) / (1 - b1))
    ldc = lt.padded(ki)
    res, forms = [], []
    for (T, Xh, pool, nr) in ((big, X, kept.astype(np.int32), giant.n_rows),
                              (small, m.triples(X, rel=m), np.arange(len(kept), dtype=np.int32), len(kept))):
        Xt = cu(Xh)
        codes = torch.empty(B * eta, dtype=torch.int32, device="cuda")
        de, dr = torch.empty(n_ce, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
        we = torch.zeros(D.apply_workspace_bytes(n_ce, nr, ki), dtype=torch.uint8, device="cuda")
        wr = torch.zeros(D.apply_workspace_bytes(B, nr, ki), dtype=torch.uint8, device="cuda")
        flags = torch.zeros(n_ce, dtype=torch.uint8, device="cuda")
        D.prepare_batch(Xt, eta, [L.SIDE_SO], len(pool), codes, de, dr, nr, nr, we, wr, entities_list=cu(pool), seed=5, counter0=2,
                        single_flags=flags if inplace else None, factored=factored)
        ce = torch.zeros(((4 if factored else 2 + eta) * B, ldc), dtype=torch.float32, device="cuda")
        cr = torch.zeros((B, ldc), dtype=torch.float32, device="cuda")
        acc = torch.zeros(1, dtype=torch.float64, device="cuda")
        spo, sno = torch.zeros(B, dtype=torch.float32, device="cuda"), torch.zeros(B * eta, dtype=torch.float32, device="cuda")
        tag_e, tag_r = torch.zeros(nr, dtype=torch.int32, device="cuda"), torch.zeros(nr, dtype=torch.int32, device="cuda")
        st = T["states"]
        ext = loss is None
        D.train_backward_ex(mid, T["ent"], T["rel"], ki, 1.0, Xt, eta, codes, ce, cr, fused_loss=-1 if ext else L.LOSS_IDS[loss], margin=1.5,
                            loss_accum=None if ext else acc, g_pos=cu(gpos) if ext else None, g_neg=cu(gneg) if ext else None,
                            scores_pos_out=None if ext else spo, scores_neg_out=None if ext else sno, single_ent=flags if inplace else None,
                            opt_id=L.OPT_IDS[opt], step=1, hyper=hyper, ent_state0=st[0], ent_state1=st[1], tag_ent=tag_e,
                            fac_ws_ent=we if factored else None)
        out = (C.c_int32 * 8)()
        L.check(lib.emg_train_backward_form(C.byref(seen[-1]), 0, out), "emg_train_backward_form")
        forms.append(list(out))
        D.apply_grouped(L.OPT_IDS[opt], T["ent"], ki, st[0], st[1], tag_e, 1, ce, n_ce, 1 if inplace else 0, hyper, we, factored=factored)
        D.apply_grouped(L.OPT_IDS[opt], T["rel"], ki, st[2], st[3], tag_r, 1, cr, B, 0, hyper, wr)
        torch.cuda.synchronize()
        res.append((acc.item(), spo, sno, codes.cpu().numpy(), int(flags.sum().item())))
    assert forms[0] == forms[1], forms
    assert forms[0][0] == (1 if loss is None else 2) and forms[0][5] == want_ip and (forms[0][6] & 1) == int(policy), forms[0]
    same_tables(kept, big, small)
    eq_bits(res[0][1], res[1][1], "raw scores of the positives"); eq_bits(res[0][2], res[1][2], "raw scores of the negatives")
    np.testing.assert_array_equal(m.codes(res[0][3]), res[1][3])
    assert res[0][4] == res[1][4] and (res[0][4] > 0) == inplace          # singletons exist and are what the in-place forms update
    assert abs(res[0][0] - res[1][0]) <= 4096 * 2.0 ** -52 * abs(res[0][0])
    Xs = m.triples(X, rel=m)
    xneg = D.corrupt_expand(cu(Xs), eta, cu(res[1][3])).cpu().numpy()
    gotE, gotR = small["ent"].cpu().numpy(), small["rel"].cpu().numpy()
    if loss is None:
        dE, dR = orc.score_grads(oname, E, R, Xs, gpos, k=kk)
        a, b = orc.score_grads(oname, E, R, xneg, gneg, k=kk)
        dE += a; dR += b
        np.testing.assert_allclose(gotE, E - lr * dE, rtol=1e-4, atol=1e-5 * max(np.abs(dE).max(), 1e-6) * lr + 1e-7)
        np.testing.assert_allclose(gotR, R - lr * dR, rtol=1e-4, atol=1e-5 * max(np.abs(dR).max(), 1e-6) * lr + 1e-7)
        return
    sp, sn = orc.score_triples(oname, E, R, Xs, k=kk), orc.score_triples(oname, E, R, xneg, k=kk)
    assert np.all(np.abs(res[0][1].cpu().numpy() - sp) <= score_tol(oname, E, R, Xs, kk))
    assert np.all(np.abs(res[0][2].cpu().numpy() - sn) <= score_tol(oname, E, R, xneg, kk))
    params = {"margin": 1.5}
    np.testing.assert_allclose(res[0][0], float(orc.loss_apply(loss, np.tile(sp, eta) if orc.REQUIRE_SAME_SIZE[loss] else sp, sn, eta, params)), rtol=1e-4)
    if opt == "sgd" and loss == "nll":
        dE, dR = orc.train_grads(oname, E, R, Xs, eta, "nll", None, [xneg], k=kk)
        np.testing.assert_allclose(gotE, E - lr * dE, rtol=2e-4, atol=2e-5 * max(np.abs(dE).max(), 1e-6) * lr + 1e-7)
        np.testing.assert_allclose(gotR, R - lr * dR, rtol=2e-4, atol=2e-5 * max(np.abs(dR).max(), 1e-6) * lr + 1e-7)
    assert np.abs(gotE - E).max() > 0


# ================================================================ sparse-giant: evaluation
def dense_tables(giant, ki, seed, plant=True):
    rs = np.random.RandomState(seed)
    n_rows = giant.n_rows
    E = (rs.randn(n_rows, ki) * 0.15).astype(F32)
    R = (rs.randn(n_rows, ki) * 0.15).astype(F32)
    if plant:       # exact ties with a probe row on rows at both sides of the marks
        p = giant.probes
        for a, b in ((1023, 1024), (2047, 2048), (4095, 4096)):
            if b < n_rows:
                E[a] = E[b]
        E[int(p[5])] = E[n_rows - 1]
    return E, R, giant.write("ent", None, E), giant.write("rel", None, R), lt.compact(E), lt.compact(R)


def eval_triples(giant, nq, seed):
    rs = np.random.RandomState(seed)
    p = giant.probes
    base = probe_triples(p, seed)
    extra = np.stack([p[rs.randint(0, len(p), nq)], p[rs.randint(0, len(p), nq)], p[rs.randint(0, len(p), nq)]], 1).astype(np.int32)
    return np.concatenate([base, extra])[:nq].copy()


@pytest.mark.parametrize("model", ["TransE_L1", "TransE_L2", "DistMult", "ComplEx"])
def test_giant_eval_pieces(giant, model):
    """emg_eval_build_queries, emg_eval_count without and with a candidate list, emg_eval_scores_dense and emg_eval_topn on
    the strided tables; every row is initialised and the twin keeps all rows and the identical ids.  (b): the committed C
    chain (oracle/c_oracle.py: build_queries, count, scores_dense), exact — the bar of
    tests/test_hip_kernels.py::test_ranks_random_embeddings_vs_canonical_oracle; top-N in (score descending, id ascending)
    order from the chain's scores."""
    L, D = libs()
    mid, oname, k, ki, scale = score_models()[model]
    E, R, Eb, Rb, Es, Rs = dense_tables(giant, ki, seed=ki + 3 * mid)
    T = eval_triples(giant, 150, seed=13)
    nq = T.shape[0]
    Qb, pb = D.eval_build_queries(mid, Eb, Rb, ki, scale, cu(T), L.EVAL_SPO)
    Qs, ps = D.eval_build_queries(mid, Es, Rs, ki, scale, cu(T), L.EVAL_SPO)
    eq_bits(Qb, Qs, "query rows"); np.testing.assert_array_equal(pb.cpu().numpy(), ps.cpu().numpy())
    Qe, pe = co.build_queries(mid, E, R, ki, scale, T, L.EVAL_SPO)
    np.testing.assert_array_equal(pb.cpu().numpy(), pe)
    cand = np.concatenate([giant.probes[::-1], np.arange(5, giant.n_rows, 7)]).astype(np.int32)
    for c in (None, cand):
        cnt = []
        for (Q, p_, Et) in ((Qb, pb, Eb), (Qs, ps, Es)):
            gt = torch.zeros(2 * nq, dtype=torch.int32, device="cuda"); eq = torch.zeros_like(gt)
            D.eval_count(mid, Q, p_, Et, ki, scale, gt, eq, cand=None if c is None else cu(c))
            cnt.append((gt.cpu().numpy(), eq.cpu().numpy()))
        np.testing.assert_array_equal(cnt[0][0], cnt[1][0]); np.testing.assert_array_equal(cnt[0][1], cnt[1][1])
        egt, eeq = co.count(mid, Qe, pe, E, ki, scale, cand=c)
        np.testing.assert_array_equal(cnt[0][0], egt); np.testing.assert_array_equal(cnt[0][1], eeq)
        assert len(set(eeq.tolist())) >= 2                # the planted ties are counted
    Sb = D.eval_scores_dense(mid, Qb[:40], Eb, ki, scale)
    eq_bits(Sb, D.eval_scores_dense(mid, Qs[:40], Es, ki, scale), "dense scores")
    chain = co.scores_dense(mid, Qe[:40], E, ki, scale)
    eq_bits(Sb, chain, "dense scores vs the chain")
    Sc = D.eval_scores_dense(mid, Qb[:40], Eb, ki, scale, cand=cu(cand))
    eq_bits(Sc, chain[:, cand], "dense scores of a candidate list")
    ib, sb = D.eval_topn(mid, Qb[:40], Eb, ki, scale, 10)
    is_, ss = D.eval_topn(mid, Qs[:40], Es, ki, scale, 10)
    np.testing.assert_array_equal(ib.cpu().numpy(), is_.cpu().numpy()); eq_bits(sb, ss, "top-N scores")
    order = np.lexsort((np.broadcast_to(np.arange(giant.n_rows), chain.shape), -chain.astype(np.float64)), axis=1)[:, :10]
    np.testing.assert_array_equal(ib.cpu().numpy(), order)
    eq_bits(sb, np.take_along_axis(chain, order, 1), "top-N scores vs the chain")


@pytest.mark.parametrize("model,precision", [("TransE_L1", 0), ("TransE_L1", 2), ("TransE_L2", 0), ("TransE_L2", 2), ("DistMult", 0),
                                             ("DistMult", 1), ("DistMult", 2), ("ComplEx", 0), ("ComplEx", 1), ("ComplEx", 2)])
def test_giant_rank_1vsall(giant, model, precision):
    """emg_rank_1vsall on the strided tables at precision modes 0, 1 (bf16 images of the strided table) and 2 (the
    half-precision / fixed-point prefilter reading the strided table into a compact image, then exact re-scoring of the
    undecided pairs against the strided rows): 280 query rows, planted ties.  (a) the twin's ranks; (b) modes 0 and 2: the ranks
    from the C chain's counts, exact (test_rank_1vsall_one_call_precision_2_equals_precision_0 holds mode 2 to mode 0).
    Mode 1 is approximate by design: (a) only."""
    L, D = libs()
    mid, oname = MID[model], model
    k = 200 if model != "ComplEx" else 100
    ki = 200
    E, R, Eb, Rb, Es, Rs = dense_tables(giant, ki, seed=ki + 5 * mid + 1)
    T = eval_triples(giant, 140, seed=17)
    Qe, pe = co.build_queries(mid, E, R, ki, 1.0, T, L.EVAL_S_O)
    egt, eeq = co.count(mid, Qe, pe, E, ki, 1.0)
    nq = T.shape[0]
    for si in range(3):
        big = D.rank_1vsall(mid, Eb, Rb, ki, 1.0, cu(T), L.EVAL_S_O, strategy=si, precision_mode=precision).cpu().numpy()
        small = D.rank_1vsall(mid, Es, Rs, ki, 1.0, cu(T), L.EVAL_S_O, strategy=si, precision_mode=precision).cpu().numpy()
        np.testing.assert_array_equal(big, small, err_msg="strategy %d" % si)
        if precision != 1:
            c = egt + eeq if si == 0 else (egt if si == 1 else egt + (eeq + 1) // 2)
            exp = np.stack([c[nq:], c[:nq]], 1) + 1          # [subject rank, object rank]; object-side rows come first
            np.testing.assert_array_equal(big, exp, err_msg="strategy %d" % si)
    assert len(set(eeq.tolist())) >= 2                    # the planted ties: the strategies differ


def cmp_int(x):
    """the comparison integers of the ranking protocol: int32(float32 score * 1e5), truncated"""
    return orc.to_cmp_int(x).astype(np.int64)


@pytest.mark.parametrize("model", ["TransE_L1", "DistMult"])
def test_giant_eval_filtered_typed_sampled_and_grid_counts(giant, model):
    """emg_eval_filter_count, emg_eval_count_lists, emg_eval_count_grouped and emg_eval_grid_count with filter entries, list
    entries, pool members and threshold entities on the probe rows of the strided table.  (b): exact integers — the C chain's
    filter counts (test_rank_1vsall_one_call_matches_python_path's bar) and counts of the comparison integers of the chain's
    dense scores (tests/test_sampled_ranking.py, tests/test_type_constraints.py, tests/test_discover_facts.py compare the same
    way)."""
    L, D = libs()
    from emgraph_amd.evaluation import FilterIndex
    mid, oname, k, ki, scale = score_models()[model]
    E, R, Eb, Rb, Es, Rs = dense_tables(giant, ki, seed=ki + 11 * mid)
    T = eval_triples(giant, 100, seed=19)
    nq, n_ent, p = T.shape[0], giant.n_rows, giant.probes
    rs = np.random.RandomState(23)
    Qe, pe = co.build_queries(mid, E, R, ki, scale, T, L.EVAL_S_O)
    I = cmp_int(co.scores_dense(mid, Qe, E, ki, scale))                         # [2 nq, n_ent]
    n_rows = 2 * nq
    # filter: known objects / subjects on probe rows
    Fl = np.concatenate([T, np.stack([np.repeat(T[:, 0], 4), np.repeat(T[:, 1], 4), p[rs.randint(0, len(p), 4 * nq)]], 1),
                         np.stack([p[rs.randint(0, len(p), 4 * nq)], np.repeat(T[:, 1], 4), np.repeat(T[:, 2], 4)], 1)]).astype(np.int32)
    ptr, idx = FilterIndex(Fl).csr(T, L.EVAL_S_O, n_ent, None)
    # lists: each row its own 40 distinct candidates (probe rows among them), padded with -1 and an id past the table
    lists = np.stack([np.concatenate([rs.choice(p, 12, replace=False), np.setdiff1d(rs.choice(n_ent, 40, replace=False), p)[:26], [-1, n_ent + 3]])
                      for _ in range(n_rows)]).astype(np.int32)
    # typed pools: three groups, rows cycling through them and through "no group"
    pools = [np.sort(rs.choice(p, 30, replace=False)), np.arange(4000, min(n_ent, 4200)), np.zeros(0, np.int64)]
    pool_ptr = np.concatenate([[0], np.cumsum([len(x) for x in pools])]).astype(np.int64)
    pool_idx = np.concatenate(pools).astype(np.int32)
    row_group = (np.arange(n_rows) % 4 - 1).astype(np.int32)
    thr = p[rs.choice(len(p), 16, replace=False)].astype(np.int32)
    res = []
    for (Et, Rt) in ((Eb, Rb), (Es, Rs)):
        Q, pos = D.eval_build_queries(mid, Et, Rt, ki, scale, cu(T), L.EVAL_S_O)
        c = torch.zeros((6, n_rows), dtype=torch.int32, device="cuda")
        D.eval_filter_count(mid, Q, pos, Et, 0, ki, scale, cu(ptr), cu(idx), c[0], c[1])
        D.eval_count_lists(mid, Q, pos, Et, ki, scale, cu(lists), c[2], c[3])
        D.eval_count_grouped(mid, Q, pos, cu(row_group), Et, ki, scale, cu(pool_ptr), cu(pool_idx), c[4], c[5])
        ggt, geq = D.eval_grid_count(mid, Q, Et, ki, scale, cu(thr))
        res.append((c.cpu().numpy(), ggt.cpu().numpy(), geq.cpu().numpy(), pos.cpu().numpy()))
    for a, b in zip(res[0], res[1]):
        np.testing.assert_array_equal(a, b)
    c, ggt, geq, pos = res[0]
    np.testing.assert_array_equal(pos, pe)
    fgt, feq = co.filter_count(mid, Qe, pe, E, 0, ki, scale, ptr, idx)
    np.testing.assert_array_equal(c[0], fgt); np.testing.assert_array_equal(c[1], feq)
    pos64 = pe.astype(np.int64)
    for r in range(n_rows):
        ids = lists[r][(lists[r] >= 0) & (lists[r] < n_ent)]
        assert c[2][r] == (I[r, ids] > pos64[r]).sum() and c[3][r] == (I[r, ids] == pos64[r]).sum(), ("lists", r)
        mem = pools[row_group[r]] if row_group[r] >= 0 else np.zeros(0, np.int64)
        assert c[4][r] == (I[r, mem] > pos64[r]).sum() and c[5][r] == (I[r, mem] == pos64[r]).sum(), ("pools", r)
    tI = I[:, thr]
    np.testing.assert_array_equal(ggt, (I[:, None, :] > tI[:, :, None]).sum(2))
    np.testing.assert_array_equal(geq, (I[:, None, :] == tI[:, :, None]).sum(2))
    assert c[2].sum() > 0 and c[4].sum() > 0 and c[0].sum() + c[1].sum() > 0


@pytest.mark.parametrize("model", ["DistMult", "ComplEx"])
def test_giant_relation_side(giant, model):
    """emg_eval_rel_scores_dense and emg_eval_rel_count against a strided relation table of 8200 rows (every row a candidate
    relation) and subjects / objects on the probe rows of the strided entity table.  (b): the object-side chain on the same
    triples, to the bit, and the counters from its comparison integers (tests/test_relation_ranking.py::check_all)."""
    L, D = libs()
    from tests import _relrank_ref as relref
    mid, oname, k, ki, scale = score_models()[model]
    E, R, Eb, Rb, Es, Rs = dense_tables(giant, ki, seed=ki + 13 * mid)
    T = eval_triples(giant, 60, seed=29)
    rows, n_rel = T.shape[0], giant.n_rows
    rs = np.random.RandomState(31)
    excl = [sorted(set(giant.probes[rs.randint(0, len(giant.probes), 5)].tolist()) | {int(pp)}) for pp in T[:, 1]]
    eptr = np.zeros(rows + 1, np.int64); eptr[1:] = np.cumsum([len(e) for e in excl])
    eidx = np.concatenate([np.asarray(e, np.int32) for e in excl])
    out = []
    for (Et, Rt) in ((Eb, Rb), (Es, Rs)):
        _, pos = D.eval_build_queries(mid, Et, Rt, ki, scale, cu(T), L.EVAL_O)
        S = D.eval_rel_scores_dense(mid, Et, Rt, ki, scale, cu(T))
        cnt = torch.zeros((4, rows), dtype=torch.int32, device="cuda")
        D.eval_rel_count(mid, Et, Rt, ki, scale, cu(T), pos, excl_ptr=cu(eptr), excl_idx=cu(eidx), cnt=cnt)
        out.append((S, cnt.cpu().numpy(), pos.cpu().numpy()))
    eq_bits(out[0][0], out[1][0], "relation-side dense scores")
    np.testing.assert_array_equal(out[0][1], out[1][1]); np.testing.assert_array_equal(out[0][2], out[1][2])
    S, cnt, pos = out[0][0].cpu().numpy(), out[0][1], out[0][2]
    # the object-side chain of (s, c, o) for 6 rows x the probe relations
    sub = np.arange(0, rows, 10)
    X = relref.expand(T[sub, 0], T[sub, 2], giant.probes)
    Qx, _ = co.build_queries(mid, E, R, ki, scale, X.astype(np.int32), L.EVAL_O)
    objs = np.unique(X[:, 2])
    chain = co.scores_dense(mid, Qx, E, ki, scale, cand=objs.astype(np.int32))
    want = relref.pick_objects(chain, T[sub, 2], len(giant.probes), objs)
    eq_bits(np.ascontiguousarray(S[sub][:, giant.probes]), np.ascontiguousarray(want), "relation side vs the object-side chain")
    C = relref.cmp_int(S)
    np.testing.assert_array_equal(C[np.arange(rows), T[:, 1]], pos)
    for got, w in zip(cnt, relref.counts(C, pos, np.arange(n_rel), excl)):
        np.testing.assert_array_equal(got, w)
    # emg_eval_rel_topn on those scores: ids past 2^13 in a row of 8200 candidates, the known relations excluded
    known = [e[:-1] if len(e) > 1 else [] for e in excl]
    kptr = np.zeros(rows + 1, np.int64); kptr[1:] = np.cumsum([len(e) for e in known])
    kidx = np.concatenate([np.asarray(e, np.int32) for e in known] + [np.zeros(0, np.int32)]).astype(np.int32)
    ti, ts = D.eval_rel_topn(out[0][0], 10, excl_ptr=cu(kptr), excl_idx=cu(kidx))
    want_i, want_s = relref.host_topn(S, np.arange(n_rel), 10, known)
    np.testing.assert_array_equal(ti.cpu().numpy(), want_i)
    np.testing.assert_array_equal(lt.bits(ts).view(np.int32), want_s)


def test_giant_prefilter_and_rescore(giant):
    """The pieces of precision mode 2 on the strided table: emg_to_f16 reads it into a compact image, emg_eval_prefilter_bounds
    reads both, emg_eval_prefilter_f16 decides what the band allows and emits the undecided (row, entity) pairs, and
    emg_eval_rescore_pairs (per pair and with the rows in LDS) / emg_eval_rescore_pairs_tiles score them exactly against the
    STRIDED rows.  The prefilter ran with re-scoring: pairs were emitted without overflow and every form added counts.
    (b): decided + re-scored counts are the C chain's, exact (tests/test_rescore.py::test_forms_agree_on_the_prefilters_own_pairs)."""
    L, D = libs()
    from emgraph_amd.evaluation import ranking as RK
    mid, k, ki = L.COMPLEX, 100, 200
    E, R, Eb, Rb, Es, Rs = dense_tables(giant, ki, seed=77)
    T = eval_triples(giant, 150, seed=37)
    n_ent = giant.n_rows
    Qe, pe = co.build_queries(mid, E, R, ki, 1.0, T, L.EVAL_S_O)
    egt, eeq = co.count(mid, Qe, pe, E, ki, 1.0)
    totals = []
    for Et, Rt in ((Eb, Rb), (Es, Rs)):
        Q, pos = D.eval_build_queries(mid, Et, Rt, ki, 1.0, cu(T), L.EVAL_S_O)
        n_rows = Q.shape[0]
        ldh = D.prefilter_ld(ki)
        Eh, Qh = D.to_f16(Et, ki, ld_dst=ldh), D.to_f16(Q, ki, ld_dst=ldh)
        band = RK.prefilter_band(Q, Qh, ki, RK.table_norm_bounds(Et, Eh, ki))
        n_seg = D.eval_prefilter_segments(n_rows, n_ent, ki)
        cap = 2048
        pairs = torch.zeros(n_seg * cap, dtype=torch.int64, device="cuda")
        pcount = torch.zeros(n_seg + 1, dtype=torch.int32, device="cuda")
        decided = torch.zeros(n_rows, dtype=torch.int32, device="cuda")
        D.eval_prefilter_f16(mid, Qh, pos, band, Eh, 0, ki, 1.0, decided, pairs, pcount)
        pc = pcount.cpu().numpy()
        assert pc[n_seg] == 0 and pc[:n_seg].max() <= cap and pc[:n_seg].sum() > 0
        forms = []
        for rps in (0, 32, "tiles"):
            c = torch.zeros((2, n_rows), dtype=torch.int32, device="cuda")
            if rps == "tiles":
                D.eval_rescore_pairs_tiles(mid, Q, pos, Et, 0, ki, 1.0, pairs, pcount, n_seg, torch.empty_like(pairs),
                                           torch.zeros(D.rescore_tiles_ws_bytes(n_ent), dtype=torch.uint8, device="cuda"), c[0], c[1])
            else:
                D.eval_rescore_pairs(mid, Q, pos, Et, 0, ki, 1.0, pairs, pcount, n_seg, c[0], c[1], D.prefilter_waves(ki), rps)
            forms.append(c.cpu().numpy())
            assert forms[-1].sum() > 0
            np.testing.assert_array_equal(forms[-1], forms[0])
        totals.append((decided.cpu().numpy() + forms[0][0], forms[0][1], Eh[:, :ki], band, pc))
    np.testing.assert_array_equal(totals[0][0], totals[1][0]); np.testing.assert_array_equal(totals[0][1], totals[1][1])
    eq_bits(totals[0][2], totals[1][2], "half image"); eq_bits(totals[0][3], totals[1][3], "band")
    np.testing.assert_array_equal(totals[0][4], totals[1][4])
    np.testing.assert_array_equal(totals[0][0], egt); np.testing.assert_array_equal(totals[0][1], eeq)


@pytest.mark.parametrize("form", ["sad", "l2", "rotate"])
def test_giant_prefilter_forms_with_rescoring(giant, form):
    """The other exact-fast forms piece by piece on the strided tables, driven as evaluation/ranking.py drives them: the
    fixed-point form of TransE-L1 (emg_eval_sad_range over both strided tables, emg_eval_sad_quantize -> the u16 image,
    emg_eval_prefilter_sad), the augmented contraction of TransE-L2 (emg_to_f16_l2 -> [e | n_hi | n_lo],
    emg_eval_prefilter_bounds, emg_eval_l2_thresholds, emg_eval_prefilter_f16_thr) and RotatE (emg_eval_rotate_image,
    emg_eval_rotate_thresholds, emg_eval_prefilter_rotate), each followed by emg_eval_rescore_pairs against the STRIDED rows (and
    by emg_eval_rescore_pairs_tiles where the form's segments allow it).  The prefilter ran with re-scoring: pairs were emitted,
    no segment overflowed, the re-scoring added counts.  (a) image bits, decided and re-scored counts equal the twin's.
    (b) decided + re-scored = the exact counts: the C chain's for TransE (test_rank_1vsall_one_call_precision_2_equals_
    precision_0's bar), the exact kernel's on the compact twin for RotatE (tests/test_rotate_fast.py's bar; that kernel is held
    to the chain in tests/test_rotate.py)."""
    L, D = libs()
    from emgraph_amd.evaluation import ranking as RK
    mid = {"sad": L.TRANSE_L1, "l2": L.TRANSE_L2, "rotate": L.ROTATE}[form]
    ki, n_ent = 200, giant.n_rows
    rs = np.random.RandomState(83 + len(form))
    E = (rs.randn(n_ent, ki) * 0.15).astype(F32)
    R = (rs.randn(n_ent, ki) * 0.15).astype(F32)
    if form == "rotate":
        R[:, ki // 2:] = 0.0
        R[:, :ki // 2] = rs.uniform(-np.pi, np.pi, (n_ent, ki // 2))
    E[1023] = E[1024]; E[4095] = E[4096]; E[int(giant.probes[5])] = E[n_ent - 1]
    Eb, Rb, Es, Rs = giant.write("ent", None, E), giant.write("rel", None, R), lt.compact(E), lt.compact(R)
    T = eval_triples(giant, 150, seed=53)
    out = []
    for Et, Rt in ((Eb, Rb), (Es, Rs)):
        fast = {"sad": lambda: RK.SadTables(Et, Rt, ki), "l2": lambda: RK.L2Tables(Et, ki), "rotate": lambda: RK.RotateTables(Et, Rt, ki)}[form]()
        assert form != "rotate" or fast.ok
        image = (fast.ent_u16 if form == "sad" else fast.ent_f16)[:, :ki + (2 if form == "l2" else 0)]      # (the columns the form defines)
        Q, pos = D.eval_build_queries(mid, Et, Rt, ki, 1.0, cu(T), L.EVAL_S_O)
        n_rows = Q.shape[0]
        n_seg, launch = fast.prepare(mid, Q, pos, 0, n_ent, 1.0, L.LINK_LINEAR)
        per = 2048 * fast.cap_factor
        pairs = torch.zeros(n_seg * per, dtype=torch.int64, device="cuda")
        pcount = torch.zeros(n_seg + 1, dtype=torch.int32, device="cuda")
        cnt = torch.zeros((2, n_rows), dtype=torch.int32, device="cuda")
        assert launch(cnt, pairs, pcount, False)
        pc = pcount.cpu().numpy()
        assert pc[n_seg] == 0 and pc[:n_seg].max() <= per and pc[:n_seg].sum() > 0
        c = torch.zeros((2, n_rows), dtype=torch.int32, device="cuda")
        D.eval_rescore_pairs(mid, Q, pos, Et, 0, ki, 1.0, pairs, pcount, n_seg, c[0], c[1], fast.waves, fast.rows)
        if fast.rows == 32:
            c2 = torch.zeros((2, n_rows), dtype=torch.int32, device="cuda")
            D.eval_rescore_pairs_tiles(mid, Q, pos, Et, 0, ki, 1.0, pairs, pcount, n_seg, torch.empty_like(pairs),
                                       torch.zeros(D.rescore_tiles_ws_bytes(n_ent), dtype=torch.uint8, device="cuda"), c2[0], c2[1])
            np.testing.assert_array_equal(c2.cpu().numpy(), c.cpu().numpy())
        assert int(c.sum().item()) > 0
        exact = torch.zeros((2, n_rows), dtype=torch.int32, device="cuda")
        D.eval_count(mid, Q, pos, Et, ki, 1.0, exact[0], exact[1])
        out.append((image, cnt[0].cpu().numpy(), c.cpu().numpy(), pc, exact.cpu().numpy(), pos.cpu().numpy(), Q))
    eq_bits(out[0][0], out[1][0], "the image of the strided table")
    for j in (1, 2, 3, 4, 5):
        np.testing.assert_array_equal(out[0][j], out[1][j])
    eq_bits(out[0][6], out[1][6], "query rows")
    decided, c, _, exact = out[0][1], out[0][2], out[0][3], out[1][4]
    np.testing.assert_array_equal(decided + c[0], exact[0]); np.testing.assert_array_equal(c[1], exact[1])
    if form != "rotate":
        Qe, pe = co.build_queries(mid, E, R, ki, 1.0, T, L.EVAL_S_O)
        egt, eeq = co.count(mid, Qe, pe, E, ki, 1.0)
        np.testing.assert_array_equal(decided + c[0], egt); np.testing.assert_array_equal(c[1], eeq)
    assert len(set(exact[1].tolist())) >= 2                      # the planted ties


def test_giant_bf16_count(giant):
    """emg_to_bf16 of the strided table, then the bf16 MFMA pieces on that image: emg_eval_pos_int_bf16 and emg_eval_count_bf16
    (all candidates and a candidate list on the probe rows).  The image's bits are held to round-to-nearest-even in
    test_giant_half_images_and_normalize; here (a): positives' integers, self ids and counts equal the twin's, and the counts of
    every row include the true entity itself (need = 0: both counters)."""
    L, D = libs()
    mid, ki, n_ent = L.DISTMULT, 200, giant.n_rows
    E, R, Eb, Rb, Es, Rs = dense_tables(giant, ki, seed=97)
    T = eval_triples(giant, 150, seed=59)
    cand = cu(np.concatenate([giant.probes[::-1], np.arange(3, n_ent, 5)]).astype(np.int32))
    out = []
    for Et, Rt in ((Eb, Rb), (Es, Rs)):
        Q, _ = D.eval_build_queries(mid, Et, Rt, ki, 1.0, cu(T), L.EVAL_S_O)
        kp = D.bf16_ld(ki)
        img, Qb = D.to_bf16(Et, ki, ld_dst=kp), D.to_bf16(Q, ki, ld_dst=kp)
        pos, self_ent = D.eval_pos_int_bf16(mid, img, ki, 1.0, cu(T), L.EVAL_S_O, Qb)
        c = torch.zeros((4, Q.shape[0]), dtype=torch.int32, device="cuda")
        D.eval_count_bf16(mid, Qb, pos, self_ent, img, ki, 1.0, c[0], c[1])
        D.eval_count_bf16(mid, Qb, pos, self_ent, img, ki, 1.0, c[2], c[3], cand=cand)
        out.append((img[:, :ki], pos.cpu().numpy(), self_ent.cpu().numpy(), c.cpu().numpy()))
    eq_bits(out[0][0], out[1][0], "bf16 image")
    for j in (1, 2, 3):
        np.testing.assert_array_equal(out[0][j], out[1][j])
    nq = T.shape[0]
    np.testing.assert_array_equal(out[0][2], np.concatenate([T[:, 2], T[:, 0]]))          # object-side rows first
    assert out[0][3][1].min() >= 1 and out[0][3][0].max() > 0 and out[0][3][0].max() < n_ent


def test_giant_calib_step(giant):
    """emg_calib_step on the strided tables: its negatives are drawn over every entity, so every row is initialised and the twin
    keeps the identical ids.  (a) the state, the drawn negatives and their scores to the bit.  (b) the negatives are
    emg_corrupt_fit's and their scores emg_score_triples' on the twin, exact (tests/test_calibration.py's step check), and those
    scores meet score_tol against the oracle."""
    L, D = libs()
    from tests import _calibration_ref as CR
    mid, oname, k, ki, scale = score_models()["DistMult"]
    E, R, Eb, Rb, Es, Rs = dense_tables(giant, ki, seed=91, plant=False)
    X = probe_triples(giant.probes, seed=47)
    B, n_ent = X.shape[0], giant.n_rows
    lp, ln = CR.labels(B, B)
    wp, wn = CR.weights(0.5, 1, 1)
    out = []
    for Et, Rt in ((Eb, Rb), (Es, Rs)):
        sp = D.score_triples(mid, Et, Rt, ki, scale, cu(X))
        dn = torch.full((B, 3), -1, dtype=torch.int32, device="cuda")
        ds = torch.full((B,), float("nan"), device="cuda")
        state = torch.zeros(8, dtype=torch.float64)
        state[1] = CR.start(B, B)[1]
        state = state.cuda()
        D.calib_step(mid, Et, Rt, ki, scale, cu(X), sp, 5, 3, lp, ln, wp, wn, state, D.calib_workspace(B, Et.device), dbg_neg=dn, dbg_scores=ds)
        out.append((state, dn.cpu().numpy(), ds, sp))
    for a, b in zip(out[0], out[1]):
        eq_bits(a, b)
    neg = D.corrupt_fit(cu(X), 1, L.SIDE_SO, entities_size=n_ent, seed=5, counter=3)
    np.testing.assert_array_equal(out[0][1], neg.cpu().numpy())
    eq_bits(out[0][2], D.score_triples(mid, Es, Rs, ki, scale, neg))
    negh = neg.cpu().numpy()
    assert np.all(np.abs(out[0][2].cpu().numpy() - orc.score_triples(oname, E, R, negh, k=k)) <= score_tol(oname, E, R, negh, k))
    assert negh[:, [0, 2]].max() > 4096 and np.any(out[0][0].cpu().numpy() != 0)          # (the state starts at zero: the step moved it)


def test_giant_discovery(giant):
    """emg_rows_within (l2), emg_rows_dbscan, emg_rows_kmeans_seed and emg_rows_kmeans over every row of the strided table.
    (b) emg_rows_within against the chain's distances, DBSCAN and k-means against their host references, all exact."""
    L, D = libs()
    from tests import _chain_ref as cr
    k, n = 20, giant.n_rows
    X = cr.blobs(n, k, seed=3)
    Xb, Xs = giant.write("ent", None, X), lt.compact(X)
    A = np.ascontiguousarray(X[giant.probes])
    dist = cr.l2_chain(A, X)
    radius = float(np.sort(dist, 1)[:, 12].mean())
    out = []
    for Xt in (Xb, Xs):
        At = Xt[cu(giant.probes)].contiguous()      # (a compact query block; the joined table is the strided one)
        count, nn_d, nn_i, pairs, pc = D.rows_within(0, At, Xt, k, -1, radius, pairs_capacity=1 << 16)
        lab, core, info = D.rows_dbscan(Xt, k, 0, 0.16, 5)          # (points of a blob lie about 0.02 sqrt(2 k) = 0.13 apart)
        centres, chosen = D.rows_kmeans_seed(Xt, k, 6, int(giant.probes[-1]), [0.1, 0.3, 0.5, 0.7, 0.9])
        moved = centres.clone()
        lab_k, kinfo = D.rows_kmeans(Xt, k, moved, 5, 1e-4)
        npairs = int(pc.cpu().numpy()[0])
        out.append((count.cpu().numpy(), nn_d, nn_i.cpu().numpy(), np.sort(pairs.cpu().numpy()[:npairs]), lab.cpu().numpy(),
                    core.cpu().numpy(), info.cpu().numpy(), centres, chosen.cpu().numpy(), lab_k.cpu().numpy(), kinfo, moved))
    for a, b in zip(out[0], out[1]):
        if hasattr(a, "detach"):
            eq_bits(a, b)
        else:
            np.testing.assert_array_equal(a, b)
    with np.errstate(invalid="ignore"):
        np.testing.assert_array_equal(out[0][0], (dist <= F32(radius)).sum(1))
    assert out[0][8][0] == giant.probes[-1] and out[0][6][0] >= 1
    # (b) DBSCAN: tests/_dbscan_ref.py on the chain's distance matrix, labels and core flags exact (tests/test_discovery_real.py);
    # k-means: tests/_kmeans_ref.py, seeding rows, labels, centres and iteration count exact (tests/test_kmeans.py)
    from tests import _kmeans_ref as KR
    from tests._dbscan_ref import dbscan_ref
    labels, core = dbscan_ref(cr.within_matrix(cr.l2_chain(X, X), 0.16), 5)
    np.testing.assert_array_equal(out[0][4], labels); np.testing.assert_array_equal(out[0][5].astype(bool), core)
    chosen, centres, _ = KR.seed(X, 6, int(giant.probes[-1]), np.array([0.1, 0.3, 0.5, 0.7, 0.9]))
    np.testing.assert_array_equal(out[0][8], chosen); eq_bits(out[0][7], centres)
    ref = KR.lloyd(X, centres, 5, 1e-4)
    np.testing.assert_array_equal(out[0][9], ref["labels"]); eq_bits(out[0][11], ref["centres"])
    inertia, n_iter, converged, tol_abs = D.kmeans_info(out[0][10])
    assert (n_iter, converged) == (ref["n_iter"], ref["converged"]) and abs(inertia - ref["inertia"]) <= n * 2.0 ** -52 * ref["inertia"]


@pytest.mark.parametrize("k", [50, 200])
def test_giant_half_images_and_normalize(giant, k):
    """emg_to_bf16 / emg_to_f16 / emg_rows_normalize reading every row of the strided table into a compact image.  (b): both
    conversions are round-to-nearest-even of each element, exact against torch's; the normalised rows against float64 at rtol
    1e-6 (a division by a float32 norm)."""
    L, D = libs()
    E, R, Eb, Rb, Es, Rs = dense_tables(giant, k, seed=k, plant=False)
    for fn, dt in ((D.to_bf16, torch.bfloat16), (D.to_f16, torch.float16)):
        big, small = fn(Eb, k)[:, :k], fn(Es, k)[:, :k]
        eq_bits(big, small, fn.__name__)
        eq_bits(big, cu(E).to(dt), fn.__name__ + " vs round-to-nearest-even")
    nb, ns = D.rows_normalize(Eb, k), D.rows_normalize(Es, k)
    eq_bits(nb, ns, "rows_normalize")
    e64 = E.astype(np.float64)
    np.testing.assert_allclose(nb.cpu().numpy(), e64 / np.sqrt((e64 ** 2).sum(1, keepdims=True)), rtol=2e-6, atol=0)


# ================================================================ many-narrow
def release_arena():
    """the file's peak is the arena plus under 1 GiB: the many-narrow cases run without it (a sparse-giant case that runs later
    takes it again)"""
    for a in _ARENAS:
        a.free()


@pytest.fixture(scope="module")
def narrow():
    libs()
    release_arena()
    t = lt.narrow_table()
    yield t
    del t
    torch.cuda.empty_cache()


def test_narrow_table_is_the_host_function(narrow):
    ids = lt.narrow_marked(n_random=4000)
    eq_bits(narrow[cu(ids)], lt.narrow_values_host(ids))
    assert narrow.shape == (lt.NARROW_ROWS, lt.NARROW_K) and narrow.stride(0) == 4


@pytest.mark.parametrize("side", ["s", "o", "s+o"])
def test_narrow_draws(side):
    """emg_corrupt_codes / emg_corrupt_fit with n_choices = 2^24 + 2^23 + 5 against the oracle's Philox stream, to the bit
    (test_corruptions_philox_bit_exact): draws above 2^24 occur, odd ones among them (lost in a float)."""
    L, D = libs()
    release_arena()
    rs = np.random.RandomState(2)
    n = lt.NARROW_ROWS
    marked = lt.narrow_marked()
    X = np.stack([marked[rs.randint(0, len(marked), 4097)], rs.randint(0, 9, 4097), marked[rs.randint(0, len(marked), 4097)]], 1).astype(np.int32)
    eta, seed, counter = 5, 2**40 + 3, 123456789012
    codes = D.corrupt_codes(X.shape[0], eta, L.SIDE_IDS[side], n, "cuda", seed=seed, counter=counter)
    exp = orc.generate_corruptions_for_fit_philox(X, eta=eta, corrupt_side=side, entities_size=n, seed=seed, counter=counter)
    got = D.corrupt_expand(cu(X), eta, codes).cpu().numpy()
    np.testing.assert_array_equal(got, exp)
    np.testing.assert_array_equal(codes.cpu().numpy(), co.corrupt_codes(X.shape[0], eta, L.SIDE_IDS[side], n, seed, counter))
    np.testing.assert_array_equal(D.corrupt_fit(cu(X), eta, L.SIDE_IDS[side], entities_size=n, seed=seed, counter=counter).cpu().numpy(), exp)
    ids = codes.cpu().numpy().astype(np.int64) & 0x7FFFFFFF
    assert ids.max() < n and (ids > (1 << 24)).sum() > 1000 and ((ids > (1 << 24)) & (ids % 2 == 1)).sum() > 500
    assert np.any(ids.astype(np.float32).astype(np.int64) != ids)


def test_narrow_candidate_draws():
    """emg_eval_draw_candidates with n_ent = 2^24 + 2^23 + 5 against tests/_sampled_ref.py::draw_rows, id for id
    (tests/test_sampled_ranking.py): ids above 2^24 occur, odd ones among them."""
    L, D = libs()
    release_arena()
    from tests import _sampled_ref as sref
    n_ent = lt.NARROW_ROWS
    for side_mode, n_q, K in ((L.EVAL_O, 130, 64), (L.EVAL_S_O, 70, 200)):
        got = D.eval_draw_candidates(n_q, 11, side_mode, K, n_ent, 2**40 + 9, "cuda").cpu().numpy()
        np.testing.assert_array_equal(got, sref.draw_rows(n_q, 11, side_mode, K, n_ent, 2**40 + 9))
        ids = got.astype(np.int64)
        assert ids.min() >= 0 and ids.max() < n_ent and ((ids > (1 << 24)) & (ids % 2 == 1)).sum() > 100


# name -> (rows, B, eta, sides, backend that must run)
GROUPING = {"sort_25m": (lt.NARROW_ROWS, 100, 5, (2,), "sort"),
            "count_25m": (lt.NARROW_ROWS, 70000, 20, (0, 1), "count"),
            "bucket_edge": (lt.BUCKET_EDGE, 70000, 20, (2,), "bucket"),
            "bucket_edge_plus_1": (lt.BUCKET_EDGE + 1, 70000, 20, (2,), "count")}


def prepare(D, pos, eta, sides, pool, n_ent, n_rel, k, watch):
    """emg_prepare_batch with negatives from ``pool``; ``watch``: fill the offset array and the bucket matrix of the entity
    workspace with 0xFF first and report which of them the call wrote"""
    B = pos.shape[0]
    n_ce = (2 + eta * len(sides)) * B
    codes = torch.empty(B * eta * len(sides), dtype=torch.int32, device="cuda")
    de = torch.empty(n_ce, dtype=torch.int32, device="cuda")
    dr = torch.empty(B, dtype=torch.int32, device="cuda")
    we = torch.zeros(D.apply_workspace_bytes(n_ce, n_ent, k), dtype=torch.uint8, device="cuda")
    wr = torch.zeros(D.apply_workspace_bytes(B, n_rel, k), dtype=torch.uint8, device="cuda")
    wrote = {}
    lay = lt.counting_layout(n_ce, n_ent) if (watch and lt.counting_backend(n_ce, n_ent)) else None
    if lay:
        assert D.apply_workspace_bytes(n_ce, n_ent) == lay["total"]
        we[lay["off"]:lay["off"] + 4 * (n_ent + 1)] = 0xFF
        if lay["bmat"] is not None:
            we[lay["bmat"]:lay["bmat"] + 4096] = 0xFF
    D.prepare_batch(cu(pos), eta, list(sides), len(pool), codes, de, dr, n_ent, n_rel, we, wr, entities_list=cu(pool), seed=5, counter0=3)
    torch.cuda.synchronize()
    if lay:
        wrote["off"] = bool((we[lay["off"]:lay["off"] + 4 * (n_ent + 1)] != 0xFF).any())
        wrote["bmat"] = lay["bmat"] is not None and bool((we[lay["bmat"]:lay["bmat"] + 4096] != 0xFF).any())
    return codes, de, dr, we, wr, n_ce, wrote


@pytest.mark.parametrize("opt", ["sgd", "adam"])
@pytest.mark.parametrize("case", sorted(GROUPING))
def test_narrow_grouping_and_apply(case, opt):
    """emg_prepare_batch + emg_apply_grouped with every destination on a marked id (both sides of 2^23 and 2^24, the last
    row), on a table of 25 165 829 rows through the sort backend (R > 16 N + 2^20) and the counting backend, on 8 388 608 rows
    through the bucket form (its last geometry: 4096 buckets of 2048 rows) and on 8 388 609 rows, where the bucket form has no
    geometry and hands over to the counting form.  WHICH BACKEND RAN: the sort backend's workspace has no per-row arrays (its
    size is below 8 bytes per row); the counting form writes the per-row offset array and not the bucket matrix, the bucket
    form the matrix and not the offsets (tables above 131072 rows) — both regions are filled with 0xFF before the call.
    (a) the twin is the gathered marked rows under the monotone remap, grouped by the counting form (the groupings are equal by
    contract: tests/test_bucket_grouping.py).  (b) keys, stable order and — rows of 16 bytes take the kernel that adds a
    segment in contribution order — the sequential float32 sums, exact (test_counting_grouping_edge_shapes); Adam: one step of
    tests/_fit_steps.py::check_step_by_step (see there)."""
    L, D = libs()
    release_arena()
    n_ent, B, eta, sides, backend = GROUPING[case]
    k, n_rel = lt.NARROW_K, 7
    marked = lt.narrow_marked(n_ent, n_random=4000)
    m = lt.Remap(marked)
    rs = np.random.RandomState(len(case) + B)
    pos = np.stack([marked[rs.randint(0, len(marked), B)], rs.randint(0, n_rel, B), marked[rs.randint(0, len(marked), B)]], 1).astype(np.int32)
    must = np.array([i for i in (0, (1 << 23) - 1, 1 << 23, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, n_ent - 1) if i < n_ent])
    pos[:len(must), 0] = must; pos[:len(must), 2] = must[::-1]      # the ids at the marks are destinations whatever the draws
    Wm = lt.narrow_values_host(marked)
    if n_ent == lt.NARROW_ROWS:
        Wb = lt.narrow_table(n_ent)
    else:
        Wb = torch.zeros((n_ent, k), dtype=torch.float32, device="cuda")
        Wb[cu(marked)] = cu(Wm)
    Ws = lt.compact(Wm)
    cb, deb, drb, web, wrb, n_ce, wrote = prepare(D, pos, eta, sides, marked.astype(np.int32), n_ent, n_rel, k, True)
    if backend == "sort":
        assert not lt.counting_backend(n_ce, n_ent) and D.apply_workspace_bytes(n_ce, n_ent) < 8 * n_ent
    else:
        assert lt.counting_backend(n_ce, n_ent)
        assert wrote == {"off": backend == "count", "bmat": backend == "bucket"}, (backend, wrote)
        assert (lt.bucket_geometry(n_ce, n_ent) is not None) == (backend == "bucket")
    cs, des, drs, wes, wrs, _, _ = prepare(D, m.triples(pos), eta, sides, np.arange(len(marked), dtype=np.int32), len(marked), n_rel, k, False)
    deb_h, des_h = deb.cpu().numpy(), des.cpu().numpy()
    np.testing.assert_array_equal(m.codes(cb.cpu().numpy()), cs.cpu().numpy())
    np.testing.assert_array_equal(m.to_small(deb_h), des_h)
    assert deb_h.max() == n_ent - 1 and deb_h.min() == 0 and (deb_h == (1 << 23) - 1).any()
    if n_ent == lt.NARROW_ROWS:
        assert ((deb_h > (1 << 24)) & (deb_h % 2 == 1)).any() and {(1 << 24) - 1, 1 << 24, (1 << 24) + 1} <= set(deb_h.tolist())
    order, nv = lt.stable_order(deb_h, n_ent)
    assert nv == n_ce
    for (ws_, dh) in ((web, deb_h), (wes, des_h)):
        keys, vals = D.apply_workspace_views(ws_, n_ce)
        np.testing.assert_array_equal(keys.cpu().numpy(), dh[order])
        np.testing.assert_array_equal(vals.cpu().numpy(), order.astype(np.int32))
    contrib = (rs.randn(n_ce, k) * 0.01).astype(F32)
    ct = cu(contrib)
    lr, mu, b1, b2, eps = 0.05, 0.9, 0.9, 0.999, 1e-7
    lr_t = lr * np.sqrt(1 - b2) / (1 - b1)
    states = []
    for (Wt, ws_) in ((Wb, web), (Ws, wes)):
        nr = Wt.shape[0]
        st = [torch.zeros_like(Wt), torch.zeros_like(Wt)] if opt == "adam" else [None, None]
        tag = torch.zeros(nr, dtype=torch.int32, device="cuda") if opt == "adam" else None
        D.apply_grouped(L.OPT_IDS[opt], Wt, k, st[0], st[1], tag, 1, ct, n_ce, 0, (lr, mu, b1, b2, eps, lr_t), ws_)
        states.append(st)
    torch.cuda.synchronize()
    sel = cu(marked)
    eq_bits(Wb[sel], Ws, "table rows of the marked ids")
    if opt == "adam":
        for j in range(2):
            eq_bits(states[0][j][sel], states[1][j], "state %d" % j)
    # rows nobody touched keep their bits (Adam's dense pass with m = v = 0 moves nothing)
    others = np.setdiff1d(np.unique(np.concatenate([marked[:-1] + 1, marked[1:] - 1, rs.randint(0, n_ent, 2000)])), marked)
    exp_others = lt.narrow_values_host(others) if n_ent == lt.NARROW_ROWS else np.zeros((len(others), k), F32)
    eq_bits(Wb[cu(others)], exp_others, "untouched rows")
    got = Ws.cpu().numpy()
    touched = np.zeros(len(marked), bool); touched[des_h] = True
    if opt == "sgd":
        sums = lt.segment_sums_f32(contrib, des_h, order, block=None)
        exact = Wm.copy()
        for r, g in sums.items():
            exact[r] = exact[r] - F32(lr) * g
        np.testing.assert_array_equal(got, exact)
    else:
        # one step of tests/_fit_steps.py::check_step_by_step: the moments inside orc.opt_apply_interval over the float64 sum +- the
        # float32 summation bound (len - 1) 2^-24 sum|c| (a segment's contributions are added one by one), 2 ulps for the last
        # roundings; the table within 4 ulps of the update the written moments give.  (The fixed rtol of
        # test_apply_rows_vs_oracle does not hold here: sums of ~700 terms cancel to ~1e-5 in a few elements, where Adam's
        # first step m / (sqrt(v) + eps) is steep in g.)
        G = np.zeros((len(marked), k), np.float64)
        A = np.zeros((len(marked), k), np.float64)
        np.add.at(G, des_h, contrib.astype(np.float64))
        np.add.at(A, des_h, np.abs(contrib).astype(np.float64))
        cnt = np.bincount(des_h, minlength=len(marked))[:, None]
        d_ = np.maximum(cnt - 1, 0) * 2.0 ** -24 * A
        iv = orc.opt_apply_interval("adam", Wm, G, d_, orc.opt_init("adam", Wm.shape), lr=lr, beta1=b1, beta2=b2, eps=eps)
        ulp = lambda x: np.spacing(np.abs(np.asarray(x, F32))).astype(np.float64)  # noqa: E731
        mv = {"m": states[1][0].cpu().numpy(), "v": states[1][1].cpu().numpy()}
        for key in ("m", "v"):
            lo, hi = iv[key]
            g64 = mv[key].astype(np.float64)
            assert np.all((g64 >= lo - 2 * ulp(lo)) & (g64 <= hi + 2 * ulp(hi))), key
        want = orc.adam_table_from_state(Wm, mv["m"], mv["v"], lr, 1, beta1=b1, beta2=b2, eps=eps).astype(np.float64)
        assert np.all(np.abs(got - want) <= 4 * ulp(want) + 4 * ulp(Wm.astype(np.float64) - want))
    assert touched.sum() >= min(len(marked) // 2, 100) and np.abs(got - Wm).max() > 0


@pytest.mark.parametrize("opt", ["sgd", "momentum", "adagrad", "adam", "adam_lazy"])
def test_narrow_trainer_step(monkeypatch, opt):
    """One Trainer.step (the package's own step: plan, fused kernels, grouping, apply) on the table of 25 165 829 rows, positives
    and the corruption pool on the marked ids.  Size-driven forms: the entity table is 400 MB, so Adam takes its DEFERRED dense
    pass by size (asserted; the twin of 4006 rows is given the same form through ``deferred_dense``), and the fused SGD kernel's
    cache-policy form would follow the table's size: EMG_CACHE_POLICY=0 pins it on both sides.  Both sides group with the
    counting form (no bucket geometry above 8 388 608 rows; the twin is below 131072 rows).  (a) tables and states of the marked
    rows to the bit, rows nobody touched unchanged.  (b) SGD, momentum, Adagrad and Adam: one step of tests/_fit_steps.py::check_step_by_step
    (orc.train_grads_bounds + orc.opt_apply_interval)."""
    L, D = libs()
    release_arena()
    from emgraph_amd.training import Trainer
    monkeypatch.setenv("EMG_CACHE_POLICY", "0")
    monkeypatch.delenv("EMG_ADAM_DEFERRED", raising=False)
    n_ent, k, ki, n_rel, B, eta, lr = lt.NARROW_ROWS, 2, lt.NARROW_K, 7, 70000, 20, 0.05
    marked, X, Wm, R, rs = _trainer_inputs()
    m = lt.Remap(marked)
    kw = dict(loss="nll", optimizer=opt, optimizer_params={"lr": lr}, batches_count=1, seed=3)
    big = Trainer(L.COMPLEX, ki, 1.0, lt.narrow_table(n_ent), R, eta, **kw)
    assert big.ent.shape[0] == n_ent and big.ent.stride(0) == ki
    assert big.deferred == (opt == "adam")                               # by size: 400 MB >= 256 MB
    small = Trainer(L.COMPLEX, ki, 1.0, Wm, R, eta, deferred_dense=big.deferred, **kw)
    for tr, Xt, pool in ((big, X, marked.astype(np.int32)), (small, m.triples(X), np.arange(len(marked), dtype=np.int32))):
        tr.set_training_set(Xt, B)
        tr.step(0, B, 1, 1, n_choices=len(pool), entities_list=cu(pool))
        assert tr.deferred == (opt == "adam")                            # the step kept the form
        tr.materialize()
    torch.cuda.synchronize()
    sel = cu(marked)
    eq_bits(big.ent[sel], small.ent, "entity rows of the marked ids")
    eq_bits(big.rel, small.rel, "relation table")
    for j in range(2):
        if big.state_ent[j] is not None:
            eq_bits(big.state_ent[j][sel], small.state_ent[j], "entity state %d" % j)
            eq_bits(big.state_rel[j], small.state_rel[j], "relation state %d" % j)
    others = np.setdiff1d(np.unique(np.concatenate([marked[:-1] + 1, marked[1:] - 1, rs.randint(0, n_ent, 2000)])), marked)
    eq_bits(big.ent[cu(others)], lt.narrow_values_host(others), "untouched rows")
    got = small.ent.cpu().numpy()
    assert np.abs(got - Wm).max() > 0
    if opt == "adam_lazy":      # (the oracle has no lazy Adam; its arithmetic is held to float64 in test_giant_apply_rows)
        return
    # (b) one step of tests/_fit_steps.py::check_step_by_step: every table and state element inside orc.opt_apply_interval over the
    # float64 gradient +- its rounding and jump allowances (orc.train_grads_bounds), +- 2 ulps of the result, of the value before
    # and of the change; Adam's table within 4 ulps of the update the written moments give
    bd = _trainer_bounds(k, eta)
    ulp = lambda x: np.spacing(np.abs(np.asarray(x, F32))).astype(np.float64)  # noqa: E731
    keys = {"sgd": [], "momentum": ["m"], "adagrad": ["acc"], "adam": ["m", "v"]}[opt]
    for tbl, W0, W1t, states in (("E", Wm, small.ent, small.state_ent), ("R", R, small.rel, small.state_rel)):
        W1 = W1t.cpu().numpy().astype(np.float64)
        st0 = orc.opt_init(opt, W0.shape)
        g, d_ = bd["d" + tbl], bd["A" + tbl] + bd["J" + tbl]
        kw = dict(lr=lr, touched=None if opt == "adam" else bd["touched_" + tbl])
        iv = orc.opt_apply_interval(opt, W0, g, d_, st0, **kw)
        pt = orc.opt_apply_interval(opt, W0, g, 0.0, st0, **kw)
        post = dict(zip(keys, [x.cpu().numpy() for x in states if x is not None]))
        for key, (lo, hi) in iv.items():
            if key == "w" and opt == "adam":
                continue
            val = W1 if key == "w" else post[key].astype(np.float64)
            prev = (W0 if key == "w" else st0[key]).astype(np.float64)
            last = 2 * (ulp(prev) + ulp(pt[key][0].astype(np.float64) - prev))
            ok = (val >= lo.astype(np.float64) - 2 * ulp(lo) - last) & (val <= hi.astype(np.float64) + 2 * ulp(hi) + last)
            assert ok.all(), (opt, tbl, key, int((~ok).sum()))
        if opt == "adam":
            want = orc.adam_table_from_state(W0, post["m"], post["v"], lr, 1).astype(np.float64)
            assert np.all(np.abs(W1 - want) <= 4 * ulp(want) + 4 * ulp(W0.astype(np.float64) - want)), tbl


_BOUNDS = {}


def _trainer_inputs():
    """the batch of test_narrow_trainer_step on the compact twin (the same seeds): (marked ids, X remapped, tables)"""
    marked = lt.narrow_marked(lt.NARROW_ROWS, n_random=4000)
    rs = np.random.RandomState(41)
    B, n_rel = 70000, 7
    X = np.stack([marked[rs.randint(0, len(marked), B)], rs.randint(0, n_rel, B), marked[rs.randint(0, len(marked), B)]], 1).astype(np.int32)
    must = np.array([0, (1 << 23) - 1, 1 << 23, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, lt.NARROW_ROWS - 1])
    X[:len(must), 0] = must; X[:len(must), 2] = must[::-1]
    return marked, X, lt.narrow_values_host(marked), (rs.randn(n_rel, lt.NARROW_K) * 0.2).astype(F32), rs


def _trainer_bounds(k, eta):
    """orc.train_grads_bounds of that batch, computed once for the optimizers that share it"""
    if "bd" not in _BOUNDS:
        marked, X, Wm, R, _ = _trainer_inputs()
        Xs = lt.Remap(marked).triples(X)
        xneg = orc.generate_corruptions_for_fit_philox(Xs, eta=eta, corrupt_side="s,o", entities_size=len(marked), seed=3, counter=0)
        with np.errstate(over="ignore", invalid="ignore"):
            _BOUNDS["bd"] = orc.train_grads_bounds("ComplEx", Wm, R, Xs, eta, "nll", None, [xneg], k=k)
    return _BOUNDS["bd"]


def plant_ties(narrow, T):
    """rows at ids on both sides of 2^24 made equal to the first queries' true objects / subjects; returns the changed ids and
    their previous rows"""
    ids = np.array([(1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 23) - 1, (1 << 23) + 1], np.int64)
    src = np.array([T[0, 2], T[0, 2], T[0, 2], T[1, 0], T[1, 0]], np.int64)
    assert not set(ids.tolist()) & set(T[:, [0, 2]].ravel().tolist())
    old = narrow[cu(ids)].clone()
    narrow[cu(ids)] = narrow[cu(src)]
    return ids, old


@pytest.mark.parametrize("model,precision", [("TransE_L1", 0), ("TransE_L1", 2), ("DistMult", 0), ("DistMult", 2)])
def test_narrow_rank_1vsall_and_topn(narrow, model, precision):
    """emg_rank_1vsall (raw and filtered through a FilterIndex whose keys hold ids above 2^24) and emg_eval_topn over 25 165 829
    candidates: 8 queries whose true entities are marked ids, exact ties planted at 2^24 - 1, 2^24, 2^24 + 1 and around 2^23 so
    that the strategies differ.  (b): ranks from the C chain's counts and filter counts, exact; top-N ids in (score
    descending, id ascending) order from the chain's scores.  The twin of a 1-vs-all entry keeps every row: here the C chain
    over the host copy of the table is that twin."""
    L, D = libs()
    from emgraph_amd.evaluation import FilterIndex
    mid, k, n_ent, n_rel = MID[model], lt.NARROW_K, lt.NARROW_ROWS, 5
    marked = lt.narrow_marked()
    hi = marked[marked > (1 << 24) + 1]
    T = np.stack([[hi[1], marked[3], hi[3], marked[-1], marked[0], hi[5], (1 << 23), hi[7]],
                  [0, 1, 2, 3, 4, 0, 1, 2],
                  [hi[0], hi[2], marked[2], marked[0], marked[-1], hi[4], hi[6], (1 << 24) + 3]], 1).astype(np.int32)
    R = (np.random.RandomState(4).randn(n_rel, k) * 0.2).astype(F32)
    Rt = lt.compact(R)
    ids, old = plant_ties(narrow, T)
    try:
        E = narrow.cpu().numpy()
        Fl = np.concatenate([T, np.stack([np.repeat(T[:, 0], 3), np.repeat(T[:, 1], 3),
                                          np.tile([(1 << 24) + 1, (1 << 24) + 7, 12345], 8)], 1)]).astype(np.int32)
        F = FilterIndex(Fl)
        ptr, idx = F.csr(T, L.EVAL_S_O, n_ent, None)
        assert idx.max() > (1 << 24)
        Qe, pe = co.build_queries(mid, E, R, k, 1.0, T, L.EVAL_S_O)
        egt, eeq = co.count(mid, Qe, pe, E, k, 1.0)
        fgt, feq = co.filter_count(mid, Qe, pe, E, 0, k, 1.0, ptr, idx)
        assert eeq[0] >= 3 and eeq[8 + 1] >= 2                  # the planted ties (object side of query 0, subject side of query 1)
        nq = 8
        for si in range(3):
            f = (lambda g, e: g + e) if si == 0 else ((lambda g, e: g) if si == 1 else (lambda g, e: g + (e + 1) // 2))
            raw = f(egt, eeq) + 1
            got = D.rank_1vsall(mid, narrow, Rt, k, 1.0, cu(T), L.EVAL_S_O, strategy=si, precision_mode=precision).cpu().numpy()
            np.testing.assert_array_equal(got, np.stack([raw[nq:], raw[:nq]], 1), err_msg="raw, strategy %d" % si)
            flt = raw - f(fgt, feq)
            got = D.rank_1vsall(mid, narrow, Rt, k, 1.0, cu(T), L.EVAL_S_O, strategy=si, filt_ptr=cu(ptr), filt_idx=cu(idx),
                                precision_mode=precision).cpu().numpy()
            np.testing.assert_array_equal(got, np.stack([flt[nq:], flt[:nq]], 1), err_msg="filtered, strategy %d" % si)
        if precision == 0:
            Q, pos_int = D.eval_build_queries(mid, narrow, Rt, k, 1.0, cu(T), L.EVAL_S_O)
            np.testing.assert_array_equal(pos_int.cpu().numpy(), pe)
            sub = [0, 1, 8, 9]                                # (four rows: 400 MB of host scores)
            ti, ts = D.eval_topn(mid, Q[sub].contiguous(), narrow, k, 1.0, 8)
            chain = co.scores_dense(mid, Qe[sub], E, k, 1.0)
            top = np.empty((4, 8), np.int64)
            for r in range(4):                               # (score descending, id ascending) without sorting 25 M entries 16 times
                kth = np.partition(chain[r], -8)[-8]
                c = np.flatnonzero(chain[r] >= kth)
                top[r] = c[np.lexsort((c, -chain[r][c].astype(np.float64)))][:8]
            np.testing.assert_array_equal(ti.cpu().numpy(), top)
            eq_bits(ts, np.take_along_axis(chain, top, 1), "top-N scores")
            # equal scores come in ascending id: the object side of query 0 ties at 2^24 - 1, 2^24, 2^24 + 1 and the true object
            tied = np.flatnonzero(chain[0] == chain[0][T[0, 2]])
            assert {(1 << 24) - 1, 1 << 24, (1 << 24) + 1, int(T[0, 2])} <= set(tied.tolist())
    finally:
        narrow[cu(ids)] = old


@pytest.mark.parametrize("model", ["TransE_L1", "DistMult"])
def test_narrow_filtered_sampled_and_typed_counts(narrow, model):
    """emg_eval_filter_count, emg_eval_count_lists and emg_eval_count_grouped (typed pools) on the table of 25 165 829 rows with
    filter entries, list entries and pool members on the marked ids — both sides of 2^23 and 2^24, odd ids above 2^24, the last
    row.  (b): counts of the comparison integers of the C chain's dense scores of the same rows, exact (the bar of
    test_giant_eval_filtered_typed_sampled_and_grid_counts); the chain over the host copy of the table is the twin of a
    1-vs-all entry, which keeps every row."""
    L, D = libs()
    mid, k, n_ent, n_rel = MID[model], lt.NARROW_K, lt.NARROW_ROWS, 5
    marked = lt.narrow_marked()
    hi = marked[marked > (1 << 24) + 1]
    T = np.array([[hi[1], 0, hi[0]], [marked[3], 1, (1 << 24) + 1], [(1 << 23), 2, marked[-1]], [marked[-1], 3, hi[4]]], np.int32)
    R = (np.random.RandomState(6).randn(n_rel, k) * 0.2).astype(F32)
    Rt = lt.compact(R)
    ids, old = plant_ties(narrow, np.array([[0, 0, T[0, 2]], [T[0, 2], 0, 0]]))       # rows at 2^24 - 1, 2^24, 2^24 + 1 := query 0's object
    try:
        E = narrow.cpu().numpy()
        Q, pos = D.eval_build_queries(mid, narrow, Rt, k, 1.0, cu(T), L.EVAL_O)
        Qe, pe = co.build_queries(mid, E, R, k, 1.0, T, L.EVAL_O)
        np.testing.assert_array_equal(pos.cpu().numpy(), pe)
        I = cmp_int(co.scores_dense(mid, Qe, E, k, 1.0))                           # [4, n_ent]
        p64 = pe.astype(np.int64)
        rs = np.random.RandomState(9)
        n_rows = 4
        members = [np.unique(np.concatenate([marked[rs.randint(0, len(marked), 20)], ids, [0, n_ent - 1]])) for _ in range(n_rows)]
        # filter CSR (ascending ids per row)
        fptr = np.concatenate([[0], np.cumsum([len(x) for x in members])]).astype(np.int64)
        fidx = np.concatenate(members).astype(np.int32)
        # lists: the members shuffled, padded with -1 and an id past the table to a common width
        width = max(len(x) for x in members) + 2
        lists = np.full((n_rows, width), -1, np.int32)
        for r, x in enumerate(members):
            lists[r, :len(x)] = rs.permutation(x)
            lists[r, -1] = n_ent + 1
        # typed pools: one group per row, one row without a group
        row_group = np.array([0, 1, -1, 2], np.int32)
        pools = [members[0], members[1], members[3]]
        pptr = np.concatenate([[0], np.cumsum([len(x) for x in pools])]).astype(np.int64)
        pidx = np.concatenate(pools).astype(np.int32)
        c = torch.zeros((6, n_rows), dtype=torch.int32, device="cuda")
        D.eval_filter_count(mid, Q, pos, narrow, 0, k, 1.0, cu(fptr), cu(fidx), c[0], c[1])
        D.eval_count_lists(mid, Q, pos, narrow, k, 1.0, cu(lists), c[2], c[3])
        D.eval_count_grouped(mid, Q, pos, cu(row_group), narrow, k, 1.0, cu(pptr), cu(pidx), c[4], c[5])
        c = c.cpu().numpy()
        fgt, feq = co.filter_count(mid, Qe, pe, E, 0, k, 1.0, fptr, fidx)
        np.testing.assert_array_equal(c[0], fgt); np.testing.assert_array_equal(c[1], feq)
        for r in range(n_rows):
            x = members[r]
            want = ((I[r, x] > p64[r]).sum(), (I[r, x] == p64[r]).sum())
            assert (c[0][r], c[1][r]) == want and (c[2][r], c[3][r]) == want, ("filter / lists", r, c[:4, r], want)
            g = row_group[r]
            want = ((I[r, pools[g]] > p64[r]).sum(), (I[r, pools[g]] == p64[r]).sum()) if g >= 0 else (0, 0)
            assert (c[4][r], c[5][r]) == want, ("pools", r, c[4:, r], want)
        assert c[1][0] >= 4 and c[3][0] >= 4 and c[5][0] >= 4       # the planted ties at 2^24 - 1, 2^24, 2^24 + 1 and the object itself
        assert max(int(x.max()) for x in members) == n_ent - 1 and any(((x > (1 << 24)) & (x % 2 == 1)).any() for x in members)
    finally:
        narrow[cu(ids)] = old


# ================================================================ sizes an entry cannot serve
def test_sizes_past_the_id_range_are_refused_with_a_message_and_write_nothing():
    """Where an entry cannot serve a size by design it says so (EMG_REQUIRE, include/emgraph_hip.h "Supported sizes") before it
    launches anything: tables declared with 2^31 rows (the C entries are called with that row count on a small buffer — the
    refusal comes before any access), an entity offset that would push top-N ids past int32, 2^31 corruption choices.  Every
    output buffer keeps its fill."""
    L, D = libs()
    import ctypes as C
    lib = L.load()
    k, big = 4, 1 << 31
    small = lt.compact(np.ones((8, k), F32))
    T = cu(np.array([[0, 0, 1], [2, 0, 3]], np.int32))
    Q, pos = D.eval_build_queries(L.DISTMULT, small, small, k, 1.0, T, L.EVAL_O)
    out = torch.full((64,), -7, dtype=torch.int32, device="cuda")
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    contrib = torch.zeros((4, k), dtype=torch.float32, device="cuda")
    cand = cu(np.zeros((2, 4), np.int32))
    with pytest.raises(L.EmgError, match="entity ids must fit int32"):
        D.eval_topn(L.DISTMULT, Q, small, k, 1.0, 2, ent_offset=(1 << 31) - 4)
    with pytest.raises(L.EmgError, match="too many rows"):
        D.prepare_batch(T, 1, [L.SIDE_SO], 8, out[:2], out[2:8], out[8:10], big, 3, ws, ws)
    with pytest.raises(L.EmgError, match="bad sizes"):
        D.group_dest(out[:4], 4, big, ws)
    with pytest.raises(L.EmgError, match="out of range"):
        D.corrupt_codes(2, 1, L.SIDE_SO, big, "cuda", out=out[:2])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    with pytest.raises(L.EmgError, match="ids must fit 31 bits"):
        L.check(lib.emg_eval_count_lists(L.DISTMULT, Q.data_ptr(), Q.stride(0), pos.data_ptr(), 2, small.data_ptr(), big, small.stride(0),
                                         cand.data_ptr(), 4, 4, None, None, k, 1.0, out[:2].data_ptr(), out[2:4].data_ptr(), stream),
                "emg_eval_count_lists")
    with pytest.raises(L.EmgError, match="too many rows"):
        L.check(lib.emg_apply_grouped(L.OPT_SGD, small.data_ptr(), big, small.stride(0), k, None, None, None, 1, contrib.data_ptr(), k, 4, 0,
                                      (C.c_float * 8)(0.1, 0, 0, 0, 0, 0, 0, 0), None, ws.data_ptr(), ws.numel(), stream), "emg_apply_grouped")
    torch.cuda.synchronize()
    assert bool((out == -7).all()) and not bool(ws.any()) and not bool(contrib.any()) and bool((small == 1).all())
