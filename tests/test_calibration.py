"""Calibration (Platt scaling) on the GPU.  Expected values come from outside the new code: tests/_calibration_ref.py (float64
numpy) on scores that device.score_triples computed for negatives that device.corrupt_fit materialised."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from emgraph_amd import _lib as L  # noqa: E402
from tests import _calibration_ref as R  # noqa: E402

F32 = np.float32
N_ENT, N_REL = 7, 3   # few entities: a replacement often is the entity it replaces


def dev():
    from emgraph_amd import device
    device.require_gpu()
    return device


def table(a):
    from emgraph_amd.training import alloc_table
    a = np.ascontiguousarray(a, dtype=F32)
    return alloc_table(a.shape[0], a.shape[1], torch.device("cuda"), init=a)


def close(got, exp, rel):
    got, exp = np.asarray(got, np.float64), np.asarray(exp, np.float64)
    return bool(np.all(np.abs(got - exp) <= rel * np.abs(exp)))


# ---------------------------------------------------------------------------------------------------------------------
# emg_calib_moments
# ---------------------------------------------------------------------------------------------------------------------
def _moments(d, sp, sn, w, b, consts):
    spt, snt = torch.from_numpy(sp).cuda(), torch.from_numpy(sn).cuda()
    ws = d.calib_workspace(len(sp) + len(sn), spt.device)
    out = torch.full((6,), float("nan"), dtype=torch.float64, device=spt.device)
    got = [d.calib_moments(spt, snt, w, b, *consts, out, ws).cpu().numpy().copy() for _ in range(2)]   # the second: re-armed
    assert got[0].tobytes() == got[1].tobytes()
    return got[0]


@pytest.mark.parametrize("n_pos,n_neg", [(1, 63), (63, 1), (64, 65), (65, 257), (257, 1000), (1000, 64)])
def test_moments_kernel_against_the_helper(n_pos, n_neg):
    d = dev()
    rs = np.random.RandomState(n_pos * 1009 + n_neg)
    consts = R.labels(n_pos, n_neg) + R.weights(0.3, n_pos, n_neg)
    cases = [(rs.normal(1.0, 2.0, n_pos), rs.normal(-1.0, 2.0, n_neg), -0.7, 0.3),
             # |w s + b| beyond 40 in both signs: the stable forms of ce and of the sigmoid
             (rs.normal(0.0, 60.0, n_pos), rs.normal(0.0, 60.0, n_neg), 1.5, -2.0),
             (np.full(n_pos, 45.0), np.full(n_neg, -45.0), -1.0, 0.25),
             # all scores equal: a singular Hessian, finite all the same
             (np.full(n_pos, 0.5), np.full(n_neg, 0.5), 0.0, R.start(n_pos, n_neg)[1])]
    for sp, sn, w, b in cases:
        sp, sn = sp.astype(F32), sn.astype(F32)
        got = _moments(d, sp, sn, w, b, consts)
        exp = R.moments(sp, sn, w, b, *consts)
        print(n_pos, n_neg, w, b, "rel err", np.abs(got - exp) / np.maximum(np.abs(exp), 1e-300))
        assert np.all(np.isfinite(got))
        assert close(got, exp, 1e-10), (got, exp)


# ---------------------------------------------------------------------------------------------------------------------
# emg_calib_step
# ---------------------------------------------------------------------------------------------------------------------
# name: (model id, k, internal k, scale)
STEP_MODELS = {"TransE_L1_k3": (L.TRANSE_L1, 3, 3, 1.0), "TransE_3_k5": (L.TRANSE_P, 5, 5, 3.0), "DistMult_k8": (L.DISTMULT, 8, 8, 1.0),
               "ComplEx_k5": (L.COMPLEX, 5, 10, 1.0), "HolE_k13": (L.HOLE, 13, 26, float(F32(2 / 13))),
               "ComplEx_k260": (L.COMPLEX, 260, 520, 1.0)}
WAVES = 4   # rows per workgroup of the step kernel: a wave each
SEED = 20240611


def _tables(name):
    mid, k, ki, scale = STEP_MODELS[name]
    rs = np.random.RandomState(sum(map(ord, name)))
    return mid, ki, scale, table(rs.normal(0, 0.6, (N_ENT, ki))), table(rs.normal(0, 0.6, (N_REL, ki)))


def _positives(n, seed):
    rs = np.random.RandomState(seed)
    return np.stack([rs.randint(0, N_ENT, n), rs.randint(0, N_REL, n), rs.randint(0, N_ENT, n)], 1).astype(np.int32)


def _run_steps(d, name, batches, counters, rate, n_pos):
    """the fused steps on ``batches`` (arrays [B, 3]) back to back — nothing between the launches — and what the existing entry
    points say about each: (state, [(negatives, their scores, debug negatives, debug scores, positive scores), ...])"""
    mid, ki, scale, ent, rel = _tables(name)
    lp, ln = R.labels(n_pos, n_pos)
    wp, wn = R.weights(rate, 1, 1)
    xs = [torch.from_numpy(b).cuda() for b in batches]
    sps = [d.score_triples(mid, ent, rel, ki, scale, x) for x in xs]
    dbg = [(torch.full((len(b), 3), -1, dtype=torch.int32, device="cuda"), torch.full((len(b),), float("nan"), device="cuda"))
           for b in batches]
    ws = d.calib_workspace(max(len(b) for b in batches), ent.device)
    state = torch.zeros(8, dtype=torch.float64)
    state[1] = R.start(n_pos, n_pos)[1]
    state = state.cuda()
    torch.cuda.synchronize()
    for x, sp, (dn, ds), c in zip(xs, sps, dbg, counters):
        d.calib_step(mid, ent, rel, ki, scale, x, sp, SEED, c, lp, ln, wp, wn, state, ws, dbg_neg=dn, dbg_scores=ds)
    torch.cuda.synchronize()
    seen = []
    for x, sp, (dn, ds), c in zip(xs, sps, dbg, counters):
        neg = d.corrupt_fit(x, 1, L.SIDE_SO, entities_size=N_ENT, seed=SEED, counter=c)
        sn = d.score_triples(mid, ent, rel, ki, scale, neg)
        seen.append((neg.cpu().numpy(), sn.cpu().numpy(), dn.cpu().numpy(), ds.cpu().numpy(), sp.cpu().numpy()))
    ticket = ws.view(torch.int32)[0].item()
    return state.cpu().numpy(), seen, ticket


def _check_steps(state, seen, ticket, n_pos, rate):
    for neg, sn, dneg, dsn, sp in seen:
        assert np.array_equal(dneg, neg)                                 # the draws of emg_corrupt_codes(B, 1, SO, n_ent, ...)
        assert dsn.view(np.int32).tolist() == sn.view(np.int32).tolist()   # bit for bit emg_score_triples
    exp = R.adam([(s[4], s[1]) for s in seen], n_pos, n_pos, rate)
    print("state", state, "helper", exp)
    assert ticket == 0                                                    # re-armed
    assert state[6] == len(seen)
    for q in range(8):
        assert abs(state[q] - exp[q]) <= 1e-6 * max(1.0, abs(exp[q])), (q, state[q], exp[q])


@pytest.mark.parametrize("name", sorted(STEP_MODELS))
@pytest.mark.parametrize("B", [1, WAVES + 1, 64, 3 * WAVES + 1])   # one row; a workgroup and a row; 64; more than three workgroups
def test_step_kernel_one_step(name, B):
    d = dev()
    X = _positives(B, 100 + B)
    state, seen, ticket = _run_steps(d, name, [X], [7], 0.25, B)
    _check_steps(state, seen, ticket, B, 0.25)


@pytest.mark.parametrize("name", sorted(STEP_MODELS))
def test_step_kernel_two_epochs_of_three_unequal_batches(name):
    """6 launches back to back on one workspace and one state record: a slot of the larger batch that a smaller one does not
    rewrite, or a ticket that is not re-armed, would show in the final state"""
    d = dev()
    X = _positives(13 + 5 + 9, 3)
    batches = [X[:13], X[13:18], X[18:]]
    counters = [e * 3 + i for e in range(2) for i in range(3)]
    state, seen, ticket = _run_steps(d, name, batches * 2, counters, 0.6, len(X))
    _check_steps(state, seen, ticket, len(X), 0.6)
    assert not np.array_equal(seen[0][0], seen[3][0])   # fresh corruptions in the second epoch


def test_step_kernel_wrong_weight_would_show():
    """the tolerance of the step tests is a thousand times below what a wrong weight moves: the helper with weight_neg = 1"""
    sp, sn = np.linspace(0.5, 2.0, 13), np.linspace(-1.0, 1.0, 13)
    a = R.adam([(sp, sn)] * 6, 13, 13, 0.25)
    b = R.adam([(sp, sn)] * 6, 13, 13, 0.5)
    assert abs(a[0] - b[0]) > 1e-3 or abs(a[1] - b[1]) > 1e-3


# ---------------------------------------------------------------------------------------------------------------------
# the public interface
# ---------------------------------------------------------------------------------------------------------------------
_FITTED = {}


def _graph():
    rs = np.random.RandomState(5)
    ents = np.array(["e%d" % i for i in range(12)])
    rels = np.array(["r%d" % i for i in range(3)])
    X = np.stack([ents[rs.randint(0, 12, 90)], rels[rs.randint(0, 3, 90)], ents[rs.randint(0, 12, 90)]], 1)
    X = np.concatenate([X, np.stack([ents, rels[np.arange(12) % 3], np.roll(ents, 1)], 1)])   # every label is seen
    return X


def fitted(kind):
    if kind not in _FITTED:
        from emgraph_amd.models import ComplEx, DistMult, HolE, TransE
        dev()
        kw = dict(k=6, epochs=3, batches_count=2, eta=2, seed=11, optimizer_params={"lr": 0.05})
        if kind == "TransE_3":
            m = TransE(embedding_model_params={"norm": 3}, **kw)
        elif kind == "ComplEx_tanh":
            m = ComplEx(embedding_model_params={"non_linearity": "tanh"}, **kw)
        else:
            m = {"TransE": TransE, "DistMult": DistMult, "ComplEx": ComplEx, "HolE": HolE}[kind](**kw)
        m.fit(_graph())
        _FITTED[kind] = m
    return _FITTED[kind]


def _raw_scores(m, X):
    from emgraph_amd.evaluation.protocol import to_idx
    d = dev()
    ent, rel = m._device_tables()
    x = torch.from_numpy(np.ascontiguousarray(to_idx(X, m.ent_to_idx, m.rel_to_idx), dtype=np.int32)).cuda()
    return x, d.score_triples(m._model_id(), ent, rel, m.internal_k, m._scale(), x)


def _sets():
    X = _graph()
    rs = np.random.RandomState(9)
    neg = X[rs.permutation(len(X))[:37]].copy()
    neg[:, 2] = X[rs.randint(0, len(X), 37), 0]
    return X[:50], neg


KINDS = ["TransE", "TransE_3", "DistMult", "ComplEx", "HolE"]


@pytest.mark.parametrize("kind", KINDS)
def test_calibrate_without_negatives_equals_the_helper_on_the_same_draws(kind):
    m = fitted(kind)
    d = dev()
    X_pos, _ = _sets()
    n_pos, bc, epochs, rate = len(X_pos), 4, 3, 0.3
    m.calibrate(X_pos, positive_base_rate=rate, batches_count=bc, epochs=epochs)
    assert m.is_calibrated and [type(p) for p in m.calibration_parameters] == [np.float32, np.float32]
    got = [p.tobytes() for p in m.calibration_parameters]
    x, sp = _raw_scores(m, X_pos)
    ent, rel = m._device_tables()
    bs = int(np.ceil(n_pos / bc))
    assert n_pos - (bc - 1) * bs not in (0, bs)   # the last batch is smaller
    batches = []
    for e in range(epochs):
        for i in range(bc):
            xb = x[i * bs:(i + 1) * bs]
            neg = d.corrupt_fit(xb, 1, L.SIDE_SO, entities_size=len(m.ent_to_idx), seed=m.seed, counter=e * bc + i)
            sn = d.score_triples(m._model_id(), ent, rel, m.internal_k, m._scale(), neg)
            batches.append((sp[i * bs:(i + 1) * bs].cpu().numpy(), sn.cpu().numpy()))
    exp = R.adam(batches, n_pos, n_pos, rate)
    w, b = [float(p) for p in m.calibration_parameters]
    print(kind, "w, b", w, b, "helper", exp[:2])
    assert abs(w - exp[0]) <= 1e-6 * max(1.0, abs(exp[0])) and abs(b - exp[1]) <= 1e-6 * max(1.0, abs(exp[1]))
    assert w != 0.0 and abs(b - R.start(n_pos, n_pos)[1]) > 1e-4   # twelve steps of about 1e-3 each
    # reproducible: the same call, the same bits
    m.calibrate(X_pos, positive_base_rate=rate, batches_count=bc, epochs=epochs)
    assert [p.tobytes() for p in m.calibration_parameters] == got


@pytest.mark.parametrize("kind", KINDS + ["ComplEx_tanh"])
def test_calibrate_with_negatives_reaches_the_helpers_minimiser(kind):
    m = fitted(kind)
    X_pos, X_neg = _sets()
    assert len(X_neg) != len(X_pos)
    _, sp = _raw_scores(m, X_pos)     # raw scores: a model with a link is calibrated on what _fn returns
    _, sn = _raw_scores(m, X_neg)
    sp, sn = sp.cpu().numpy(), sn.cpu().numpy()
    found = {}
    for rate in (None, 0.2, 0.8):
        m.calibrate(X_pos, X_neg, positive_base_rate=rate)
        got = [p.tobytes() for p in m.calibration_parameters]
        w, b = [float(p) for p in m.calibration_parameters]
        pi = rate if rate is not None else len(X_pos) / (len(X_pos) + len(X_neg))
        ew, eb = R.newton(sp, sn, len(X_pos), len(X_neg), pi)
        print(kind, rate, "w, b", w, b, "helper", ew, eb)
        assert abs(w - ew) <= 1e-5 * abs(ew) and abs(b - eb) <= 1e-5 * abs(eb)
        found[rate] = (w, b)
        m.calibrate(X_pos, X_neg, positive_base_rate=rate)   # a second call replaces the first with the same bits
        assert [p.tobytes() for p in m.calibration_parameters] == got
    # a higher base rate weighs the negatives less: probabilities go up, i.e. the logit's offset -b goes up
    assert found[0.8][1] < found[None][1] < found[0.2][1]


@pytest.mark.parametrize("kind", ["TransE", "ComplEx", "ComplEx_tanh"])
def test_predict_proba(kind):
    m = fitted(kind)
    X_pos, X_neg = _sets()
    m.calibrate(X_pos, X_neg)
    w, b = [np.float64(p) for p in m.calibration_parameters]
    X = np.concatenate([X_pos, X_neg])
    _, raw = _raw_scores(m, X)
    raw = raw.cpu().numpy().astype(np.float64)
    p = m.predict_proba(X)
    assert p.dtype == np.float32 and p.shape == (len(X),)
    assert np.abs(p - 1.0 / (1.0 + np.exp(w * raw + b))).max() <= 1e-6
    assert (p >= 0).all() and (p <= 1).all()
    assert m._predict_proba(X).tobytes() == p.tobytes()
    if kind == "ComplEx_tanh":   # the link is predict's alone
        assert np.abs(m.predict(X) - np.tanh(raw)).max() < 1e-6
    from emgraph_amd.evaluation.protocol import to_idx
    idx = to_idx(X, m.ent_to_idx, m.rel_to_idx)
    assert m.predict_proba(idx, from_idx=True).tobytes() == p.tobytes()
    with pytest.raises(ValueError, match="entities"):
        m.predict_proba(np.array([["e0", "r0", "nobody"]]))
    with pytest.raises(ValueError, match="relations"):
        m.predict_proba(np.array([["e0", "nothing", "e1"]]))
    # extreme scores stay inside [0, 1]
    d = dev()
    s = torch.tensor([-1e30, -100.0, 0.0, 100.0, 1e30], dtype=torch.float32, device="cuda")
    q = d.calib_proba(s, -2.0, 0.5).cpu().numpy()
    assert np.all(np.isfinite(q)) and q[0] == 0.0 and q[-1] == 1.0 and abs(q[2] - 1 / (1 + np.exp(0.5))) < 1e-7


def test_calibration_round_trip_through_a_checkpoint(tmp_path):
    from emgraph_amd.utils.model_utils import restore_model, save_model
    m = fitted("DistMult")
    X_pos, X_neg = _sets()
    m.calibrate(X_pos, X_neg)
    p = m.predict_proba(X_pos)
    path = str(tmp_path / "m.pkl")
    save_model(m, path)
    r = restore_model(path)
    assert r.is_calibrated and [np.asarray(a).tobytes() for a in r.calibration_parameters] == [a.tobytes() for a in m.calibration_parameters]
    assert r.predict_proba(X_pos).tobytes() == p.tobytes()
