"""Losses and score links on the device where they are hard: the kinks (TF's MaximumGrad: x >= y), the inclusive +-75 clip and the
first float outside it, expf past +-88.7 and below -104, the softplus link's 9999 e^x reaching inf, 1 - s^2 and s (1 - s) at
saturation, a multiclass ratio that underflows, a one-hot softmax, and NaN under every loss.

tests/_loss_edge_ref.py holds the grid, the literal float32 restatement (the CLASS of every element), the float64 one (its
VALUE) and the per-element budget, derived on the host from +-1 ulp on every libm result (tests/test_loss_edges_host.py prints
it).  Hinge gradients and every element whose budget is zero are compared with ==; the loss sum in three launches (moderate,
saturated, non-finite: rtol 2e-5 of the absolute float64 sum for the first two, by class for the third); the only quantity not
asserted is the gradient at a score that is itself NaN.  Every test prints how many elements it compared with ==, within budget
and by class.

(a) the standalone kernels (emg_loss, emg_link_scores, emg_link_grads) on the scores themselves;
(b) the fused kernel on DESIGNED scores: probe tables — entity i = (v_i, 0, ..), u = (1, 0, ..), relation r = (1, 0, ..) (TransE:
    u = r = 0, so that (s + r) - o is v_i exactly), positives (e_a, r, u), hand-made codes that replace the subject by e_b — make
    the positive score v_a and the negative score v_b, and column 0 of the contribution rows dL/dscore itself (TransE-L2: through
    (g / |v|) v, restated in float32).  A value a model does not reproduce exactly is dropped for it by that comparison;
    The matrix is a stated choice: every model at every form with the linear link; in-place SGD with no singleton flagged on
    DistMult and TransE-L1 at 16 lanes and a wave per group; links and edge weights on DistMult and ComplEx at those two forms (the
    loss code is one function, instantiated per form: what varies with the form is how a group's lanes share it).
(c) fit() raises "Loss is" for a NaN score under each loss (losses/utils.py:49: tf.clip_by_value hands the NaN on;
    EmbeddingModel.py:1422 raises).
"""
import ctypes as C

import numpy as np
import pytest

from tests import _focuse_ref as fref
from tests import _loss_edge_ref as ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32 = np.float32
WEIGHTS = np.array([0, 2.0 ** -20, 0.5, 1], F32)
_CACHE = {}


def _dev():
    from emgraph_amd import _lib as L
    from emgraph_amd import device as d
    d.require_gpu()
    return L, d


def cu(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _expect(name, params, pos, neg, eta, n_sides=1):
    """loss_expect, computed once per input"""
    key = (name, tuple(sorted(params.items())), pos.tobytes(), neg.tobytes(), eta, n_sides)
    if key not in _CACHE:
        _CACHE[key] = ref.loss_expect(name, pos, neg, eta, params, n_sides)
    return _CACHE[key]


def dev_loss(name, params, pos, neg, eta, n_sides=1):
    L, d = _dev()
    acc = torch.zeros(1, dtype=torch.float64, device="cuda")
    gp, gn = d.loss(L.LOSS_IDS[name], cu(pos, F32), cu(neg, F32), len(pos), eta, n_sides, float(params.get("margin", 1.0)),
                    float(params.get("alpha", 0.5)), acc)
    return float(acc.item()), gp.cpu().numpy(), gn.cpu().numpy()


def same(got, want, what=""):
    """equal by value, NaN where NaN"""
    np.testing.assert_array_equal(np.asarray(got, F32), np.asarray(want, F32), err_msg=what)


class Tally:
    def __init__(self):
        self.eq = self.bud = self.cls = self.finite = 0
        self.chain = 0      # fused gradients compared with == against the standalone chain of the same scores

    def add(self, e, got, what):
        a, b, c = e.check(got, what)
        self.eq, self.bud, self.cls = self.eq + a, self.bud + b, self.cls + c
        self.finite += int(np.isfinite(e.lit).sum())

    def close(self, what):
        print("%s: %d compared with ==, %d within budget, %d by class%s" % (
            what, self.eq, self.bud, self.cls, "; %d with == against the standalone chain" % self.chain if self.chain else ""))
        assert self.eq + self.bud >= 0.95 * self.finite, (what, self.eq, self.bud, self.finite)


def check_loss_launches(run, name, params, pos, neg, eta, n_sides, what, pos64=None, neg64=None):
    """the three launches of the loss sum; run(mask) -> the device's sum over the groups of the mask; pos / neg: the float32
    scores the loss sees, pos64 / neg64 their float64 values (default: the same)"""
    masks = ref.split_groups(name, pos, neg, eta, params, n_sides)
    p64 = pos.astype(np.float64) if pos64 is None else pos64
    n64 = neg.astype(np.float64) if neg64 is None else neg64
    for label, m in zip(("moderate", "saturated", "non-finite"), masks):
        if not m.any():
            continue
        got = run(m)
        if label == "non-finite":
            p, n = ref.take_groups(pos, neg, eta, n_sides, m)
            want = ref.class_of_sum(ref.terms32(name, p, n, eta, params, n_sides))
            print("%s %s launch: %d groups, device %r, class %d" % (what, label, m.sum(), got, want))
            assert int(ref.classify(got)) == want, (what, label, got, want)
        else:
            s, a = ref.loss_sum64(name, p64[m], n64.reshape(n_sides, eta, -1)[:, :, m].reshape(-1), eta, params, n_sides)
            print("%s %s launch: %d groups, device %r, float64 %r (absolute sum %r)" % (what, label, m.sum(), got, s, a))
            assert np.isfinite(got) and abs(got - s) <= 2e-5 * a, (what, label, got, s, a)


# ------------------------------------------------------------------------------------------------
# (a) the standalone kernels
# ------------------------------------------------------------------------------------------------
FINITE_SHAPES = [("all pairs", ref.all_pairs, 1, 1), ("eta 3, two sides", lambda: ref.drawn(3, 2), 3, 2),
                 ("eta 70", lambda: ref.drawn(70, 1), 70, 1)]
NONFINITE_SHAPES = [("non-finite pairs", ref.nonfinite_pairs, 1, 1), ("non-finite eta 3", lambda: ref.nonfinite_drawn(3), 3, 1)]


@pytest.mark.parametrize("cfg", range(len(ref.LOSS_CONFIGS)), ids=["%s-%s" % (n, "-".join("%g" % v for v in p.values())) for n, p in ref.LOSS_CONFIGS])
def test_loss_kernel_on_the_grid(cfg):
    name, params = ref.LOSS_CONFIGS[cfg]
    tally = Tally()
    for label, make, eta, n_sides in FINITE_SHAPES + NONFINITE_SHAPES:
        pos, neg = make()
        what = "%s %s: %s" % (name, params, label)
        ep, en = _expect(name, params, pos, neg, eta, n_sides)
        _, gp, gn = dev_loss(name, params, pos, neg, eta, n_sides)
        tally.add(ep, gp, what + " g_pos")
        tally.add(en, gn, what + " g_neg")

        def run(mask):
            p, n = ref.take_groups(pos, neg, eta, n_sides, mask)
            return dev_loss(name, params, p, n, eta, n_sides)[0]
        check_loss_launches(run, name, params, pos, neg, eta, n_sides, what)
    tally.close("%s %s" % (name, params))


@pytest.mark.parametrize("cfg", range(len(ref.LOSS_CONFIGS)), ids=["%s-%s" % (n, "-".join("%g" % v for v in p.values())) for n, p in ref.LOSS_CONFIGS])
def test_every_non_finite_pair_contributes_its_class_to_the_loss(cfg):
    """one launch per pair (B = 1): a NaN score's contribution is NaN under every loss (losses/utils.py:49), an infinite term is
    inf with its sign, everything else finite"""
    L, d = _dev()
    name, params = ref.LOSS_CONFIGS[cfg]
    pos, neg = ref.nonfinite_pairs()
    want = ref.classify(ref.terms32(name, pos, neg, 1, params))
    acc = torch.zeros(len(pos), dtype=torch.float64, device="cuda")
    sp, sn = cu(pos), cu(neg)
    gp, gn = torch.empty(1, dtype=torch.float32, device="cuda"), torch.empty(1, dtype=torch.float32, device="cuda")
    for i in range(len(pos)):
        d.loss(L.LOSS_IDS[name], sp[i:i + 1], sn[i:i + 1], 1, 1, 1, float(params.get("margin", 1.0)), float(params.get("alpha", 0.5)),
               acc[i:i + 1], gp, gn)
    got = ref.classify(acc.cpu().numpy())
    bad = got != want
    nan_scores = np.isnan(pos) | np.isnan(neg)
    assert (want[nan_scores] == 3).all()
    print("%s %s: %d pairs by class (%d NaN, %d inf)" % (name, params, len(pos), (want == 3).sum(), ((want == 1) | (want == 2)).sum()))
    assert not bad.any(), "%s: class of the loss differs for (pos, neg) = %s: device %s, literal float32 %s" % (
        name, list(zip(pos[bad][:6], neg[bad][:6])), got[bad][:6], want[bad][:6])


def dev_link(link, w, sw, pos, neg, eta_total):
    """emg_link_scores on copies: (effective pos, effective neg, factor pos, factor neg)"""
    L, d = _dev()
    sp, sn = cu(pos, F32), cu(neg, F32)
    fp, fn = d.link_scores(L.LINK_IDS[link], cu(w, F32) if w is not None else None, sw, sp, sn, len(pos), eta_total)
    return sp.cpu().numpy(), sn.cpu().numpy(), fp.cpu().numpy(), fn.cpu().numpy()


@pytest.mark.parametrize("link", ref.LINKS)
def test_link_kernels_on_the_grid(link):
    L, d = _dev()
    tally = Tally()
    n = len(ref.FULL)
    pos = np.repeat(ref.FULL, len(WEIGHTS)).astype(F32)                    # every value under every edge weight
    w = np.tile(WEIGHTS, n).astype(F32)
    B, eta = len(pos), 2
    neg = np.concatenate([np.roll(pos, 1), np.roll(pos, 7)]).astype(F32)
    for weights, sw in ((None, 0.0), (w, 0.0), (w, 0.25), (w, 1.0)):
        what = "%s weights=%s sw=%g" % (link, weights is not None, sw)
        wp = ref.weight32(sw, w, True) if weights is not None else None
        wn = ref.weight32(sw, np.tile(w, eta), False) if weights is not None else None
        sp, sn, fp, fn = dev_link(link, weights, sw, pos, neg, eta)
        for (es, ed), s, f, side in ((ref.link_expect(link, pos, wp), sp, fp, "pos"), (ref.link_expect(link, neg, wn), sn, fn, "neg")):
            tally.add(es, s, what + " value " + side)
            tally.add(ed, f, what + " factor " + side)
        # emg_link_grads: one float32 product with the factor
        gp0, gn0 = np.roll(pos, 3), np.roll(neg, 5)
        gp, gn = cu(gp0), cu(gn0)
        d.link_grads(gp, gn, cu(fp), cu(fn), B, eta)
        with np.errstate(all="ignore"):
            same(gp.cpu().numpy(), gp0 * fp, what)
            same(gn.cpu().numpy(), gn0 * fn, what)
    tally.close("link " + link)


# ------------------------------------------------------------------------------------------------
# (b) the fused kernel on designed scores
# ------------------------------------------------------------------------------------------------
CINT = C.c_int32
LINKED = 2
# name -> (columns per row (per half for the complex models), EMG_WIDE_GROUPS, (W, NV, LPG))
FORMS = {"16 lanes": (4, "0", (4, 1, 16)), "32 lanes": (128, "0", (4, 1, 32)), "wave, 1 chunk": (4, "1", (4, 1, 64)),
         "wave, 2 chunks": (512, "1", (4, 2, 64)), "scalar": (5, "1", (1, 1, 64))}
MODELS = ["DistMult", "ComplEx", "HolE", "TransE_L1", "TransE_L2"]
FUSED_LOSSES = [("pairwise", {"margin": 1.0}), ("nll", {}), ("absolute_margin", {"margin": 1.0})]


class _Spy:
    """the library with emg_train_backward_ex preceded by its dry run (emg_train_backward_form): which form ran"""

    def __init__(self, lib):
        self._lib, self.form = lib, None

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def emg_train_backward_ex(self, a, stream):
        out = (CINT * 8)()
        assert self._lib.emg_train_backward_form(a, 0, out) == 0, self._lib.emg_last_error()
        self.form = list(out)
        return self._lib.emg_train_backward_ex(a, stream)


def _through(model, g, v):
    """column 0 of the contribution row of a score v whose dL/dscore is g, as the kernel forms it (float32)"""
    g, v = np.asarray(g, F32), np.asarray(v, F32)
    with np.errstate(all="ignore"):
        if model == "TransE_L1":          # -(g sgn(d)), d = v <= 0
            return np.where(v < 0, g, -(g * F32(0))).astype(F32)
        if model == "TransE_L2":          # -((g / |v|) v); a zero norm takes no gradient
            return np.where(v < 0, -((g / np.abs(v)) * v), F32(0)).astype(F32)
    return g


class Probe:
    def __init__(self, model, cols, monkeypatch, wide):
        from emgraph_amd.training import alloc_table
        from oracle import emgraph_oracle as orc
        self.L, self.d = _dev()
        monkeypatch.setenv("EMG_WIDE_GROUPS", wide)
        monkeypatch.delenv("EMG_CACHE_POLICY", raising=False)
        self.spy = _Spy(self.L.load())
        monkeypatch.setattr(self.L, "load", lambda: self.spy)
        self.model, self.mid = model, orc.MODEL_IDS[model]
        cplx, transe = model in ("ComplEx", "HolE"), model.startswith("TransE")
        values = ref.FULL if model == "DistMult" else (ref.GRID[ref.GRID <= 0] if transe else np.concatenate([ref.GRID, [F32(-0.0)]]))
        self.ki = 2 * cols if cplx else cols
        n = len(values)
        E, R = np.zeros((n + 1, self.ki), F32), np.zeros((1, self.ki), F32)
        E[:n, 0] = values
        E[n, 0] = R[0, 0] = 0.0 if transe else 1.0
        self.E0, self.R0, self.u = E, R, n
        self.dev = torch.device("cuda")
        self.Et, self.Rt = alloc_table(n + 1, self.ki, self.dev, init=E), alloc_table(1, self.ki, self.dev, init=R)
        # which values the model reproduces exactly: by comparison, not by a list
        idx = np.arange(n)
        out = self.run(idx, idx[None, :], "pairwise", {"margin": 1.0}, check_scores=False)
        with np.errstate(invalid="ignore"):
            keep = ((out["sp"] == values) | (np.isnan(out["sp"]) & np.isnan(values))) & ((out["sn"] == values) | (np.isnan(out["sn"]) & np.isnan(values)))
        self.idx = idx[keep]
        self.V = values[keep]
        must = np.concatenate([-ref.MUST_KEEP, [] if transe else ref.MUST_KEEP]).astype(F32)
        missing = [v for v in must if v not in self.V]
        assert not missing, "%s does not reproduce %s" % (model, missing)
        print("%s: probe keeps %d of %d values (dropped %s)" % (model, keep.sum(), n, values[~keep]))

    def run(self, a, b, name, params, link="linear", w=None, sw=0.0, inplace=False, check_scores=True):
        """positives (e_a, r, u), negatives (e_b, r, u); a [B], b [eta, B] index the probe's entity rows"""
        L, d, dev = self.L, self.d, self.dev
        a, b = np.asarray(a), np.asarray(b)
        B, eta = len(a), b.shape[0]
        n_ce = (2 + eta) * B
        pos = cu(np.stack([a, np.zeros(B, np.int64), np.full(B, self.u)], 1), np.int32)
        codes = cu(b.reshape(-1), np.int32)                       # bit 31 clear: the SUBJECT is replaced
        ce = torch.full((n_ce, self.ki), float("nan"), dtype=torch.float32, device=dev)
        cr = torch.full((B, self.ki), float("nan"), dtype=torch.float32, device=dev)
        acc = torch.zeros(1, dtype=torch.float64, device=dev)
        sp = torch.empty(B, dtype=torch.float32, device=dev)
        sn = torch.empty(B * eta, dtype=torch.float32, device=dev)
        kw = {}
        if inplace:   # plain in-place SGD with no singleton flagged: truthful, every row of the batch occurs at least twice
            rows, counts = np.unique(np.concatenate([a, b.reshape(-1), np.full(B, self.u)]), return_counts=True)
            assert counts.min() >= 2
            kw = dict(single_ent=torch.zeros(n_ce, dtype=torch.uint8, device=dev), opt_id=L.OPT_SGD, step=1,
                      hyper=(0.1, 0.9, 0.9, 0.999, 1e-7, 0.1), tag_ent=torch.zeros(self.u + 1, dtype=torch.int32, device=dev))
        d.train_backward_ex(self.mid, self.Et, self.Rt, self.ki, 1.0, pos, eta, codes, ce, cr, fused_loss=L.LOSS_IDS[name],
                            margin=float(params.get("margin", 1.0)), loss_accum=acc, scores_pos_out=sp, scores_neg_out=sn,
                            link=L.LINK_IDS[link], edge_w=cu(w, F32) if w is not None else None, sw=sw, **kw)
        out = dict(sp=sp.cpu().numpy(), sn=sn.cpu().numpy(), gp=ce[:B, 0].cpu().numpy(), gn=ce[2 * B:, 0].cpu().numpy(),
                   loss=float(acc.item()), form=self.spy.form)
        if check_scores:
            same(out["sp"], self.E0[a, 0], "designed positive scores")
            same(out["sn"], self.E0[b.reshape(-1), 0], "designed negative scores")
        if inplace:
            same(self.Et.cpu().numpy(), self.E0, "no singleton flagged: the table is untouched")
        return out

    def shapes(self):
        """(label, a, b): eta = 1 over all pairs of kept values; eta = 3 and eta = 70 drawn, B = 3 x the kept values"""
        nv = len(self.idx)
        yield "all pairs", np.repeat(self.idx, nv), np.tile(self.idx, nv)[None, :]
        for eta in (3, 70):
            rs = np.random.RandomState(eta)
            a = np.tile(self.idx, 3)
            b = self.idx[rs.randint(0, nv, (eta, len(a)))]
            for g, v in ((0, -0.5), (1, -1e4), (2, -3e38)):       # planted groups: negatives all equal (where the model keeps the value)
                at = np.flatnonzero(self.V == F32(v))
                if len(at):
                    b[:, g] = self.idx[at[0]]
            yield "eta %d" % eta, a, b


def check_fused(pr, label, a, b, name, params, tally, link="linear", w=None, sw=0.0, inplace=False, form=None, ip=0):
    eta, B = b.shape[0], len(a)
    what = "%s %s %s link=%s weights=%s sw=%g: %s" % (pr.model, name, params, link, w is not None, sw, label)
    raw_p, raw_n = pr.E0[a, 0], pr.E0[b.reshape(-1), 0]
    out = pr.run(a, b, name, params, link, w, sw, inplace)
    if form is not None:
        linked = link != "linear" or w is not None
        assert tuple(out["form"][2:5]) == form and out["form"][5] == ip and bool(out["form"][6] & LINKED) == linked, (what, out["form"])
    # the standalone chain on the same scores: the same __device__ functions, the same bits
    L, d = pr.L, pr.d
    if link != "linear" or w is not None:
        eff_p, eff_n, fp, fn = dev_link(link, w, sw, raw_p, raw_n, eta)
    else:
        eff_p, eff_n, fp, fn = raw_p, raw_n, None, None
    _, gp, gn = dev_loss(name, params, eff_p, eff_n, eta)
    if fp is not None:
        with np.errstate(all="ignore"):
            gp, gn = (gp * fp).astype(F32), (gn * fn).astype(F32)
    unasserted = np.isnan(raw_n)
    same(np.where(unasserted, 0, out["gn"]), np.where(unasserted, 0, _through(pr.model, gn, raw_n)), what + " g_neg against the standalone chain")
    unasserted = np.isnan(raw_p)
    same(np.where(unasserted, 0, out["gp"]), np.where(unasserted, 0, _through(pr.model, gp, raw_p)), what + " g_pos against the standalone chain")
    tally.chain += int((~np.isnan(raw_n)).sum() + (~np.isnan(raw_p)).sum())
    if fp is None:   # and against the references directly, where column 0 carries dL/dscore untouched
        ep, en = _expect(name, params, raw_p, raw_n, eta)
        if pr.model != "TransE_L2":
            carried_p, carried_n = (raw_p < 0, raw_n < 0) if pr.model == "TransE_L1" else (np.ones(B, bool), np.ones(B * eta, bool))
            for e, got, carried, side in ((ep, out["gp"], carried_p, " g_pos"), (en, out["gn"], carried_n, " g_neg")):
                sub = ref.Expect(e.lit[carried], e.want[carried], e.tol[carried], e.ulps[carried], e.skip[carried])
                tally.add(sub, got[carried], what + side)

    # the loss: three launches
    if link != "linear" or w is not None:
        wp = ref.weight32(sw, w, True) if w is not None else None
        wn = ref.weight32(sw, np.tile(w, eta), False) if w is not None else None
        lit_p, lit_n = ref.link32(link, raw_p, wp)[0], ref.link32(link, raw_n, wn)[0]
        with np.errstate(all="ignore"):
            p64, n64 = fref.link(link, raw_p)[0], fref.link(link, raw_n)[0]
            if w is not None:
                w64p, w64n = fref.weights(w, F32(sw).astype(np.float64))
                p64, n64 = w64p * p64, np.tile(w64n, eta) * n64
    else:
        lit_p, lit_n, p64, n64 = raw_p, raw_n, None, None

    def run(mask):
        return pr.run(a[mask], b[:, mask], name, params, link, w[mask] if w is not None else None, sw)["loss"]
    check_loss_launches(run, name, params, lit_p, lit_n, eta, 1, what, p64, n64)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("model", MODELS)
def test_fused_kernel_on_designed_scores(monkeypatch, model, form):
    cols, wide, shape = FORMS[form]
    pr = Probe(model, cols, monkeypatch, wide)
    tally = Tally()
    for name, params in FUSED_LOSSES:
        for label, a, b in pr.shapes():
            check_fused(pr, label, a, b, name, params, tally, form=shape)
    tally.close("%s, %s" % (model, form))


@pytest.mark.parametrize("form", ["16 lanes", "wave, 1 chunk"])
@pytest.mark.parametrize("model", ["DistMult", "TransE_L1"])
def test_fused_kernel_in_place_sgd_with_no_singleton(monkeypatch, model, form):
    """single_ent given, every flag zero: the same bits as without it, the table untouched"""
    cols, wide, shape = FORMS[form]
    pr = Probe(model, cols, monkeypatch, wide)
    tally = Tally()
    for name, params in FUSED_LOSSES:
        for label, a, b in pr.shapes():
            check_fused(pr, label, a, b, name, params, tally, inplace=True, form=shape, ip=1)
    tally.close("%s, %s, in place" % (model, form))


@pytest.mark.parametrize("link", ref.LINKS)
@pytest.mark.parametrize("form", ["16 lanes", "wave, 1 chunk"])
@pytest.mark.parametrize("model", ["DistMult", "ComplEx"])
def test_fused_kernel_links_and_edge_weights(monkeypatch, model, form, link):
    cols, wide, shape = FORMS[form]
    pr = Probe(model, cols, monkeypatch, wide)
    tally = Tally()
    for name, params in FUSED_LOSSES:
        for label, a, b in pr.shapes():
            w = np.tile(WEIGHTS, -(-len(a) // len(WEIGHTS)))[:len(a)].astype(F32)
            for weights, sw in ((None, 0.0), (w, 0.0), (w, 0.25), (w, 1.0)):
                if link == "linear" and weights is None:
                    continue                                     # (test_fused_kernel_on_designed_scores)
                check_fused(pr, label, a, b, name, params, tally, link, weights, sw, form=shape)
    # (the standalone chain is held to the references in (a); nothing here is compared within a budget)
    tally.close("%s, %s, link %s" % (model, form, link))


# ------------------------------------------------------------------------------------------------
# (c) fit()
# ------------------------------------------------------------------------------------------------
TOY = np.array([["a", "y", "b"], ["b", "y", "a"], ["a", "y", "c"], ["c", "y", "a"], ["a", "y", "d"], ["c", "y", "d"],
                ["b", "y", "c"], ["f", "y", "e"]])


@pytest.mark.parametrize("loss", ["pairwise", "nll", "absolute_margin", "self_adversarial", "multiclass_nll"])
def test_fit_raises_on_a_nan_score(loss):
    """one NaN in an entity row the training set uses: the reference's loss is NaN under every loss (tf.clip_by_value and
    tf.maximum hand it on) and its fit loop raises (EmbeddingModel.py:1422)"""
    from emgraph_amd.models import DistMult
    _dev()
    ent0 = np.full((6, 4), 0.5, F32)
    ent0[0, 1] = np.nan
    rel0 = np.full((1, 4), 0.5, F32)
    m = DistMult(k=4, epochs=1, batches_count=1, loss=loss, optimizer="sgd", initializer="constant",
                 initializer_params={"entity": ent0, "relation": rel0})
    with pytest.raises(ValueError, match="Loss is"):
        m.fit(TOY)
