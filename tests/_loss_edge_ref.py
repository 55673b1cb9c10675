"""Losses and score links where they are hard — kinks, clip bounds, saturation, non-finite scores: the score grid, two
restatements of the reference, and the per-element error budget the device is held to.

THE GRID (float32, symmetric about zero, 43 values): 0, +-2^-140 (denormal), +-2^-20, +-0.5, +-1, +-1.5, +-2, +-3, +-10, +-73, +-74,
+-prev(75), +-75, +-next(75), +-76 (the +-75 clip of losses/utils.py:44-53, inclusive), +-79, +-80 (9999 e^x passes float32 at 79.52),
+-88, +-89 (e^x passes float32 at 88.72), +-104 (e^x is 0 below -103.97), +-1e4, +-3e38.  NONFINITE: -0.0, +-inf, NaN.

RESTATEMENT 1, literal float32 (grads32, terms32, link32): the formulas op for op in numpy float32, every libm call going through
a Libm object.  It gives the CLASS of every element (finite, +-inf, NaN) and the per-group loss term.  Sums run in the order the
formulas are written (a positive's eta equal NLL terms one after the other; the multiclass denominator from the positive on);
NLL's gradients in the forms 1 / (1 + e^pos) and e / (1 + e), e = e^neg.
  losses: pairwise.py:66-70, nll.py:55-59, absolute_margin.py:66-70, self_adversarial.py:90-112, nll_multiclass.py:70-81; their
  gradients are the analytic ones of oracle.loss_grads (tf.maximum's goes to x where x >= y; clip_by_value's is 1 inside the
  INCLUSIVE bounds); tf.clip_by_value and tf.maximum propagate NaN (losses/utils.py:49)
  links: EmbeddingModel.py:679-722, 801-816 and custom_softplus :90-96; tanh' = 1 - y^2 and sigmoid' = y (1 - y) from the output.
RESTATEMENT 2, float64 (grads64, oracle._loss_terms64, tests/_focuse_ref.link): the VALUE wherever the literal form is finite.
grads64 keeps the formulas of oracle.loss_grads in float64 to the end.  The self-adversarial loss forms its exponents from
float32 scores in float32 — fl(alpha neg - max), fl(neg + margin), fl(margin + pos) — and that rounding belongs to the operation on
float32 inputs, so the exponents enter the float64 restatement as float32 forms them.

THE BUDGET of an element (never taken from device output): the literal chain is evaluated with the result of every libm call
(exp, log / log1p, tanh; for the multiclass loss the positive's exp and the negatives' exp separately) moved by -1, 0 and +1 ulp
from its correctly rounded value — at most 3^3 combinations, each applied to every element alike.  The budget is the largest
distance of any of these from the float64 value plus one ulp of the magnitude below for the final rounding.  +-1 ulp is the
bound assumed for the device's expf / logf / log1pf / tanhf: no larger documented one was at hand, and tests/test_link_ranking.py
sweeps the same functions exhaustively for order.  Where the chain holds no libm call (hinge gradients, the linear link) or
every perturbed value is the same small integer as the float64 value (0 outside the clip, a saturated softplus' derivative 1),
the budget is zero and the comparison ==.
One departure, for the two losses that sum over a group (self-adversarial, multiclass): a pattern that moves every term of a sum
alike cancels in term / sum and leaves every addition of the sum rounding as before, while on the device each call errs on its
own and each moved term changes how the later additions round.  So SCATTERED = 128 seeded patterns are added that move every
element of every call independently by -1, 0 or +1: what the perturbed sums span, in place of the worst-case bound of a sum taken in
order (eta / 2 ulp).  The budgets stay below 16 ulp with them (figures below).
The unit is the ulp of the cancellation-free magnitude: |g| itself for NLL; gm of oracle._loss_grad_bounds for self-adversarial
and multiclass (w (dell + a ell + a sum w ell); |g| + softmax(pos)); for the links 1 for tanh' and softplus', y for sigmoid',
max(|y|, 1) for softplus (log(1 + e) rounds 1 + e), |y| otherwise, times the FocusE weight.

LARGEST BUDGETS on the shapes of tests/test_loss_edges.py, in ulps of the unit, as tests/test_loss_edges_host.py prints them (it
holds every one below 16 where the expected gradient is a normal float; softmax_weight_normal: a self-adversarial gradient whose
softmax numerator is denormal is as short of bits as a denormal gradient and is left out of that bound, not of its budget):
    pairwise 0, absolute_margin 0 (==); nll g_pos 13.04 (eta = 70 equal terms summed in order), g_neg 2.38 (the unperturbed chain:
    0.67); self_adversarial g_pos 3.61, g_neg 12.08; multiclass_nll g_pos 2.00, g_neg 11.09;
    links, value / derivative: linear 0 / 0 (with weights 1.50 / 0), tanh 2.47 / 3.07 (3.07 / 5.14), sigmoid 3.36 / 3.19
    (3.62 / 3.62), softplus 2.60 / 1.43 (3.50 / 2.12).
"""
import itertools

import numpy as np

from oracle import emgraph_oracle as orc
from tests import _focuse_ref as fref

F32 = np.float32
_P75, _N75 = np.nextafter(F32(75), F32(0)), np.nextafter(F32(75), F32(np.inf))
_HALF = np.array([2.0 ** -140, 2.0 ** -20, 0.5, 1, 1.5, 2, 3, 10, 73, 74, _P75, 75, _N75, 76, 79, 80, 88, 89, 104, 1e4, 3e38], F32)
GRID = np.concatenate([-_HALF[::-1], [F32(0)], _HALF]).astype(F32)
NONFINITE = np.array([-0.0, np.inf, -np.inf, np.nan], F32)
FULL = np.concatenate([GRID, NONFINITE]).astype(F32)
MUST_KEEP = np.array([0, 0.5, 1, 1.5, 2, 3, 10, 73, 74, _P75, 75, _N75, 76], F32)   # a fused probe keeps these on the side(s) it reaches

LOSS_CONFIGS = [("pairwise", {"margin": 1.0}), ("nll", {}), ("absolute_margin", {"margin": 1.0}),
                ("self_adversarial", {"margin": 3.0, "alpha": 0.5}), ("self_adversarial", {"margin": 1.0, "alpha": 0.5}),
                ("self_adversarial", {"margin": 3.0, "alpha": 1.0}), ("self_adversarial", {"margin": 1.0, "alpha": 1.0}),
                ("multiclass_nll", {})]
LINKS = fref.LINKS
KINDS = {"pairwise": (), "absolute_margin": (), "nll": ("exp",), "self_adversarial": ("exp", "log"),
         "multiclass_nll": ("exp", "exp_pos"), "linear": (), "tanh": ("tanh",), "sigmoid": ("exp",), "softplus": ("exp", "log")}


def _cr(f, x):
    """the correctly rounded float32 result (through float64): a function within 1 ulp of the truth lands on it or beside it"""
    with np.errstate(all="ignore"):
        return f(np.asarray(x, F32).astype(np.float64)).astype(F32)


class Libm:
    """float32 libm: the correctly rounded result moved by d[kind] ulps — or, with `rs`, every element of every call moved
    independently by -1, 0 or +1 (exact zeros, infinities and NaN stay)"""

    def __init__(self, rs=None, **d):
        self.d, self.rs = d, rs

    def _move(self, y, kind):
        y = np.asarray(y, F32)
        d = self.rs.randint(-1, 2, y.shape) if self.rs is not None else self.d.get(kind, 0)
        if self.rs is None and d == 0:
            return y
        with np.errstate(all="ignore"):
            z = np.where(np.asarray(d) > 0, np.nextafter(y, F32(np.inf)), np.where(np.asarray(d) < 0, np.nextafter(y, F32(-np.inf)), y))
        return np.where(np.isfinite(y) & np.isfinite(z) & (y != 0), z, y).astype(F32)

    def exp(self, x, kind="exp"):
        return self._move(_cr(np.exp, x), kind)

    def log(self, x):
        return self._move(_cr(np.log, x), "log")

    def log1p(self, x):
        return self._move(_cr(np.log1p, x), "log")

    def tanh(self, x):
        return self._move(_cr(np.tanh, x), "tanh")


SCATTERED = 128   # seeded patterns on top of the 3^k uniform ones, for the two losses that sum over a group


def perturbations(kinds, scattered=0):
    for deltas in itertools.product((-1, 0, 1), repeat=len(kinds)):
        yield Libm(**dict(zip(kinds, deltas)))
    for i in range(scattered):
        yield Libm(rs=np.random.RandomState(4242 + i))


def _clip(v):
    return np.clip(v, F32(-75), F32(75)).astype(F32)       # (np.clip, as tf.clip_by_value, hands a NaN on)


def _in75(v):
    return ((v >= F32(-75)) & (v <= F32(75))).astype(F32)


def _relu(v):
    return np.maximum(v, F32(0)).astype(F32)                # (np.maximum, as tf.maximum, hands a NaN on)


def _log_sigmoid(x, lm):
    """tf.math.log_sigmoid = -softplus(-x), the stable form"""
    return (-(np.fmax(-x, F32(0)) + lm.log1p(lm.exp(-np.abs(x))))).astype(F32)


def _shape(pos, neg, eta, n_sides):
    pos = np.asarray(pos, F32)
    return pos, np.asarray(neg, F32).reshape(n_sides, eta, pos.shape[0])


def grads32(name, pos, neg, eta, params=None, n_sides=1, lm=None):
    """literal float32 (dL/dpos [B], dL/dneg [n_sides * eta * B]); neg is side-major, then eta-major"""
    lm = lm or Libm()
    p = params or {}
    pos, negr = _shape(pos, neg, eta, n_sides)
    B = pos.shape[0]
    gp, gn = np.zeros(B, F32), np.zeros(negr.shape, F32)
    one = F32(1)
    with np.errstate(all="ignore"):
        if name == "nll":
            pc = _clip(pos)
            gp1 = -_in75(pos) * (one / (one + lm.exp(pc)))
        if name == "self_adversarial":
            m, a = F32(p.get("margin", orc.DEFAULT_MARGIN_ADVERSARIAL)), F32(p.get("alpha", orc.DEFAULT_ALPHA_ADVERSARIAL))
        for sd in range(n_sides):
            nr = negr[sd]
            if name == "pairwise":
                act = (((F32(p.get("margin", 1.0)) - pos)[None, :] + nr) >= 0).astype(F32)
                gn[sd] = act
                for j in range(eta):
                    gp = gp - act[j]
            elif name == "absolute_margin":
                gn[sd] = ((F32(p.get("margin", 1.0)) + nr) >= 0).astype(F32)
                for j in range(eta):
                    gp = gp - one
            elif name == "nll":
                e = lm.exp(_clip(nr))
                gn[sd] = _in75(nr) * (e / (one + e))
                for j in range(eta):
                    gp = gp + gp1
            elif name == "self_adversarial":
                gp = gp - one / (one + lm.exp(m + pos))
                mx = np.full(B, -np.inf, F32)
                for j in range(eta):
                    mx = np.fmax(mx, a * nr[j])
                w = [lm.exp(a * nr[j] - mx) for j in range(eta)]
                ell = [_log_sigmoid(-nr[j] - m, lm) for j in range(eta)]
                den, wsum = np.zeros(B, F32), np.zeros(B, F32)
                for j in range(eta):
                    den = den + w[j]
                    wsum = wsum + w[j] * ell[j]
                sbar = wsum / den
                for j in range(eta):
                    wn = w[j] / den
                    dell = -(one / (one + lm.exp(-(nr[j] + m))))
                    gn[sd, j] = -(wn * dell + (a * wn) * (ell[j] - sbar))
            elif name == "multiclass_nll":
                pe = lm.exp(_clip(pos), "exp_pos")
                en = [lm.exp(_clip(nr[j])) for j in range(eta)]
                den = pe
                for j in range(eta):
                    den = den + en[j]
                gp = gp + (-(one - pe / den) * _in75(pos))
                for j in range(eta):
                    gn[sd, j] = _in75(nr[j]) * en[j] / den
            else:
                raise ValueError(name)
    return gp.astype(F32), gn.reshape(-1).astype(F32)


def terms32(name, pos, neg, eta, params=None, n_sides=1, lm=None):
    """literal float32 loss term of every group [B] (summed over its negatives and sides, in that order)"""
    lm = lm or Libm()
    p = params or {}
    pos, negr = _shape(pos, neg, eta, n_sides)
    t = np.zeros(pos.shape[0], F32)
    one = F32(1)
    with np.errstate(all="ignore"):
        for sd in range(n_sides):
            nr = negr[sd]
            if name == "pairwise":
                for j in range(eta):
                    t = t + _relu((F32(p.get("margin", 1.0)) - pos) + nr[j])
            elif name == "absolute_margin":
                for j in range(eta):
                    t = t + (_relu(F32(p.get("margin", 1.0)) + nr[j]) - pos)
            elif name == "nll":
                tp = lm.log(one + lm.exp(-_clip(pos)))
                for j in range(eta):
                    t = t + (tp + lm.log(one + lm.exp(_clip(nr[j]))))
            elif name == "self_adversarial":
                m, a = F32(p.get("margin", orc.DEFAULT_MARGIN_ADVERSARIAL)), F32(p.get("alpha", orc.DEFAULT_ALPHA_ADVERSARIAL))
                t = t + (-_log_sigmoid(m + pos, lm))
                mx = np.full(pos.shape[0], -np.inf, F32)
                for j in range(eta):
                    mx = np.fmax(mx, a * nr[j])
                den, wsum = np.zeros_like(t), np.zeros_like(t)
                for j in range(eta):
                    w = lm.exp(a * nr[j] - mx)
                    den = den + w
                    wsum = wsum + w * _log_sigmoid(-nr[j] - m, lm)
                t = t - wsum / den
            elif name == "multiclass_nll":
                pe = lm.exp(_clip(pos), "exp_pos")
                den = pe
                for j in range(eta):
                    den = den + lm.exp(_clip(nr[j]))
                t = t + (-lm.log(pe / den))
            else:
                raise ValueError(name)
    return t.astype(F32)


def classify(x):
    """0 finite, 1 +inf, 2 -inf, 3 NaN"""
    x = np.asarray(x)
    return np.where(np.isnan(x), 3, np.where(np.isposinf(x), 1, np.where(np.isneginf(x), 2, 0)))


def grads64(name, pos, neg, eta, params=None, n_sides=1):
    """restatement 2: (g_pos, g_neg, gm_pos, gm_neg) in float64 — the formulas of oracle.loss_grads (whose values it reproduces,
    tests/test_loss_edges_host.py) kept in float64 to the end, and the cancellation-free magnitudes of oracle._loss_grad_bounds.
    The self-adversarial loss FORMS its exponents from float32 scores in float32 (alpha neg - max, neg + margin, margin + pos): that
    rounding is part of the operation on float32 inputs, so the exponents enter here as float32 forms them"""
    pos, negr = _shape(pos, neg, eta, n_sides)
    p = params or {}
    B = pos.shape[0]
    gp, gmp, gn, gmn = np.zeros(B), np.zeros(B), [], []
    zero = np.zeros(B), np.zeros(eta * B)
    lo, hi = orc.DEFAULT_CLIP_EXP_LOWER, orc.DEFAULT_CLIP_EXP_UPPER
    p64 = pos.astype(np.float64)
    with np.errstate(all="ignore"):
        for sd in range(n_sides):
            (a, b), (ma, mb), _, _ = orc._loss_grad_bounds(name, pos, negr[sd].reshape(-1), eta, params, zero[0], zero[1],
                                                           lambda s: -1.0 + 0 * s)
            a, b = a.astype(np.float64), b.astype(np.float64)
            n64 = negr[sd].astype(np.float64)
            if name == "nll":
                a = -eta * ((p64 >= lo) & (p64 <= hi)) / (1.0 + np.exp(np.clip(p64, lo, hi)))
                b = (((n64 >= lo) & (n64 <= hi)) / (1.0 + np.exp(-np.clip(n64, lo, hi)))).reshape(-1)
            elif name == "multiclass_nll":
                ep, en = np.exp(np.clip(p64, lo, hi)), np.exp(np.clip(n64, lo, hi))
                den = en.sum(0) + ep
                a = -(1.0 - ep / den) * ((p64 >= lo) & (p64 <= hi))
                b = ((en / den[None, :]) * ((n64 >= lo) & (n64 <= hi))).reshape(-1)
            elif name == "self_adversarial":
                m32, a32 = F32(p.get("margin", orc.DEFAULT_MARGIN_ADVERSARIAL)), F32(p.get("alpha", orc.DEFAULT_ALPHA_ADVERSARIAL))
                al = float(a32)
                z = (a32 * negr[sd]).astype(F32)
                z = (z - np.fmax.reduce(z, axis=0, keepdims=True)).astype(np.float64)      # fl(alpha neg - max)
                w = np.exp(z)
                w = w / w.sum(0, keepdims=True)
                ell = -np.logaddexp(0.0, -(-negr[sd] - m32).astype(np.float64))             # log_sigmoid(fl(-neg - margin))
                dell = -1.0 / (1.0 + np.exp(-(negr[sd] + m32).astype(np.float64)))           # -sigmoid(fl(neg + margin))
                sbar = (w * ell).sum(0, keepdims=True)
                a = -1.0 / (1.0 + np.exp((m32 + pos).astype(np.float64)))                    # -sigmoid(-fl(margin + pos))
                b = (-(w * dell + al * w * (ell - sbar))).reshape(-1)
            gp, gmp = gp + a, gmp + ma
            gn.append(b)
            gmn.append(mb)
    return gp, np.concatenate(gn), gmp, np.concatenate(gmn)


def softmax_weight_normal(name, pos, neg, eta, params=None, n_sides=1):
    """mask over g_neg: the element's softmax numerator exp(fl(alpha neg - max)) is 0 or a NORMAL float.  A denormal one (exponent
    below -87.3) carries fewer than 24 bits, so a gradient formed from it — itself a normal float just above 2^-126 — cannot be
    within a few ulps of its magnitude in any float32 implementation; such elements keep their absolute budget and are left out of
    the 16-ulp bound, as gradients that are denormal themselves are.  All true for the other losses."""
    pos, negr = _shape(pos, neg, eta, n_sides)
    if name != "self_adversarial":
        return np.ones(negr.size, bool)
    a32 = F32((params or {}).get("alpha", orc.DEFAULT_ALPHA_ADVERSARIAL))
    with np.errstate(all="ignore"):
        z = (a32 * negr).astype(F32)
        e = np.exp((z - np.fmax.reduce(z, axis=1, keepdims=True)).astype(np.float64))
    return ~((e > 0) & (e < np.finfo(F32).tiny)).reshape(-1)


def ulp_of(mag):
    with np.errstate(all="ignore"):
        m = np.where(np.isfinite(mag), np.abs(mag), 0.0)
        return np.spacing(np.minimum(m, 3e38).astype(F32)).astype(np.float64)


def _budget(lit, want, mag, candidates, no_libm=False):
    """(tol [abs], ulps): largest distance of a candidate from `want` where both are finite, plus one ulp of `mag`"""
    maxd = np.zeros(want.shape)
    with np.errstate(all="ignore"):
        for c in candidates:
            dist = np.abs(c.astype(np.float64) - want)
            maxd = np.fmax(maxd, np.where(np.isfinite(dist), dist, 0.0))
    u = ulp_of(mag)
    # == where no libm call is in the chain at all, or where every candidate is the same small integer (0 and +-1 above all)
    exact = (maxd == 0) & (lit.astype(np.float64) == want) & (no_libm | ((want == np.round(want)) & (np.abs(want) < 2 ** 24)))
    tol = np.where(exact, 0.0, maxd + u)
    return tol, tol / u


class Expect:
    """what one array of device results is held to: lit (float32, the class), want (float64), tol (absolute; 0: ==), ulps (tol in
    ulps of the cancellation-free magnitude), skip (not asserted: the gradient at a score that is itself NaN)"""

    def __init__(self, lit, want, tol, ulps, skip):
        self.lit, self.want, self.tol, self.ulps, self.skip = lit, want, tol, ulps, skip

    def finite(self):
        return np.isfinite(self.lit) & ~self.skip

    def check(self, got, what=""):
        """asserts; returns (compared with ==, within budget, by class)"""
        got = np.asarray(got, F32)
        assert got.shape == self.lit.shape, (what, got.shape, self.lit.shape)
        fin = self.finite()
        byclass = ~np.isfinite(self.lit) & ~self.skip
        bad = byclass & (classify(got) != classify(self.lit))
        assert not bad.any(), "%s: class differs at %s: got %s, literal float32 %s" % (what, np.flatnonzero(bad)[:8], got[bad][:8], self.lit[bad][:8])
        eq = fin & (self.tol == 0)
        bad = eq & ~(got.astype(np.float64) == self.want)
        assert not bad.any(), "%s: not equal at %s: got %s, want %s" % (what, np.flatnonzero(bad)[:8], got[bad][:8], self.want[bad][:8])
        bud = fin & (self.tol != 0)
        with np.errstate(all="ignore"):
            err = np.abs(got.astype(np.float64) - self.want)
        bad = bud & ~(err <= self.tol)
        assert not bad.any(), "%s: past the budget at %s: got %s, want %s, budget %s" % (
            what, np.flatnonzero(bad)[:8], got[bad][:8], self.want[bad][:8], self.tol[bad][:8])
        return int(eq.sum()), int(bud.sum()), int(byclass.sum())


def loss_expect(name, pos, neg, eta, params=None, n_sides=1):
    """(Expect of g_pos, Expect of g_neg)"""
    pos, negr = _shape(pos, neg, eta, n_sides)
    lit_p, lit_n = grads32(name, pos, neg, eta, params, n_sides)
    wp, wn, mp, mn = grads64(name, pos, neg, eta, params, n_sides)
    if name in ("nll",):
        mp, mn = np.abs(wp), np.abs(wn)
    cand = [grads32(name, pos, neg, eta, params, n_sides, lm)
            for lm in perturbations(KINDS[name], SCATTERED if name in ("self_adversarial", "multiclass_nll") else 0)]
    tp, up = _budget(lit_p, wp, mp, [c[0] for c in cand], not KINDS[name])
    tn, un = _budget(lit_n, wn, mn, [c[1] for c in cand], not KINDS[name])
    # a NaN score's own gradient is not asserted; under the two losses that normalise over the group a NaN anywhere makes
    # every gradient of the group NaN in both restatements (asserted by class)
    return (Expect(lit_p, wp, tp, up, np.isnan(pos)), Expect(lit_n, wn, tn, un, np.isnan(negr).reshape(-1)))


# ---- links ----
def weight32(sw, w, positive):
    one, sw, w = F32(1), F32(sw), np.asarray(w, F32)
    return (sw + (one - sw) * ((one - w) if positive else w)).astype(F32)    # :716-722


def link32(name, x, weight=None, lm=None):
    """literal float32 (weight * phi(x), weight * phi'(x))"""
    lm = lm or Libm()
    x = np.asarray(x, F32)
    one = F32(1)
    with np.errstate(all="ignore"):
        if name == "linear":
            s, d = x, np.ones_like(x)
        elif name == "tanh":
            s = lm.tanh(x)
            d = one - s * s
        elif name == "sigmoid":
            s = one / (one + lm.exp(-x))
            d = s * (one - s)
        elif name == "softplus":
            e = F32(9999) * lm.exp(x)
            s = lm.log(one + e)
            d = one - one / (one + e)
        else:
            raise ValueError("Invalid non-linearity")
        if weight is not None:
            s, d = weight * s, weight * d
    return s.astype(F32), d.astype(F32)


def link_expect(name, x, weight=None):
    """(Expect of the effective score, Expect of the factor); weight float32 [n] or None"""
    x = np.asarray(x, F32)
    lit_s, lit_d = link32(name, x, weight)
    with np.errstate(all="ignore"):
        y, dy = fref.link(name, x)
        ms = np.maximum(np.abs(y), 1.0) if name == "softplus" else np.abs(y)
        md = {"linear": np.ones_like(y), "tanh": np.ones_like(y), "sigmoid": np.abs(y), "softplus": np.ones_like(y)}[name]
        if weight is not None:
            w64 = weight.astype(np.float64)
            y, dy, ms, md = w64 * y, w64 * dy, np.abs(w64) * ms, np.abs(w64) * md
    cand = [link32(name, x, weight, lm) for lm in perturbations(KINDS[name])]
    ts, us = _budget(lit_s, y, ms, [c[0] for c in cand], not KINDS[name])
    td, ud = _budget(lit_d, dy, md, [c[1] for c in cand], not KINDS[name])
    skip = np.isnan(x)
    return Expect(lit_s, y, ts, us, skip), Expect(lit_d, dy, td, ud, skip)


# ---- shapes (the whole workload of tests/test_loss_edges.py) ----
def all_pairs(values=GRID):
    """eta = 1 over every (pos, neg) pair: B = len(values)^2 (43^2 = 1849: 7 blocks of 256 and a ragged one)"""
    n = len(values)
    return np.repeat(values, n).astype(F32), np.tile(values, n).astype(F32)


def drawn(eta, n_sides=1, seed=0, B=129):
    """B = 129 positives (the grid three times over), negatives drawn from the grid; group 0's negatives all equal, group 1's
    softmax one-hot (one negative at 1e4 among -1e4), group 2's all -3e38"""
    rs = np.random.RandomState(1000 * eta + 10 * n_sides + seed)
    pos = np.tile(GRID, -(-B // len(GRID)))[:B].astype(F32)
    negr = GRID[rs.randint(0, len(GRID), (n_sides, eta, B))].astype(F32)
    negr[:, :, 0] = F32(0.5)
    negr[:, :, 1] = F32(-1e4)
    negr[:, eta // 2, 1] = F32(1e4)
    negr[:, :, 2] = F32(-3e38)
    return pos, negr.reshape(-1)


def nonfinite_pairs():
    """eta = 1: every pair with a non-finite score (or -0.0) on at least one side"""
    a = [(p, n) for p in FULL for n in NONFINITE] + [(p, n) for p in NONFINITE for n in GRID]
    return np.array([x[0] for x in a], F32), np.array([x[1] for x in a], F32)


def nonfinite_drawn(eta=3, seed=0, B=129):
    """drawn() with one negative of every group replaced by a non-finite value (or -0.0), and non-finite positives in the last groups"""
    rs = np.random.RandomState(77 + seed)
    pos, neg = drawn(eta, 1, seed, B)
    negr = neg.reshape(eta, B).copy()
    negr[rs.randint(0, eta, B), np.arange(B)] = NONFINITE[np.arange(B) % 4]
    pos = pos.copy()
    pos[-4:] = NONFINITE
    return pos, negr.reshape(-1)


def split_groups(name, pos, neg, eta, params=None, n_sides=1):
    """the three launches of the loss sum: masks over the groups — moderate (every score within +-10), saturated but finite, and
    those whose literal float32 term is not finite or that hold a non-finite score"""
    pos, negr = _shape(pos, neg, eta, n_sides)
    allv = np.concatenate([pos[None, :], negr.reshape(-1, pos.shape[0])])
    t = terms32(name, pos, neg, eta, params, n_sides)
    third = ~np.isfinite(allv).all(0) | ~np.isfinite(t)
    with np.errstate(invalid="ignore"):
        moderate = ~third & (np.abs(allv) <= 10).all(0)
    return moderate, ~third & ~moderate, third


def take_groups(pos, neg, eta, n_sides, mask):
    pos, negr = _shape(pos, neg, eta, n_sides)
    return pos[mask].copy(), negr[:, :, mask].reshape(-1).copy()


def loss_sum64(name, pos, neg, eta, params=None, n_sides=1):
    """(float64 sum, absolute sum) of oracle._loss_terms64 over the sides"""
    pos, negr = _shape(pos, neg, eta, n_sides)
    s = a = 0.0
    for sd in range(n_sides):
        x, y = orc._loss_terms64(name, pos, negr[sd].reshape(-1), eta, params)
        s, a = s + x, a + y
    return s, a


def class_of_sum(terms):
    """the class a sum of these float32 terms has, in any order (NaN if any is NaN or both infinities occur)"""
    with np.errstate(all="ignore"):
        return int(classify(np.sum(np.asarray(terms, np.float64))))
