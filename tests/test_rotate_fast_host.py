"""RotatE exact-fast ranking without a device: the residual / band / threshold arithmetic of csrc/emg_rank_rotate.hip restated in
numpy (tests/_rotate_fast_ref.py) against float64, a sweep of single-coordinate worst cases, what 'auto' resolves to, the ABI table
and the refusals that stay."""
import os
import re

import numpy as np
import pytest

from emgraph_amd import _lib as L
from tests import _rotate_fast_ref as ref
from tests import _rotate_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32

NEW_SYMBOLS = {"emg_eval_rotate_ld": 1, "emg_eval_rotate_image": 11, "emg_eval_rotate_thresholds": 10,
               "emg_eval_prefilter_rotate_segments": 2, "emg_eval_prefilter_rotate": 15, "emg_eval_prefilter_rotate_dense": 11}


def _check_band(q, e, k_int):
    """the band holds for the emulated prefilter in both subnormal behaviours it allows, against the float64 sum of the f32 operands
    AND against the canonical f32 chain; the thresholds decide no pair wrongly"""
    n = k_int // 2
    s = ref.image_scale(float(np.abs(e).max()))
    assert np.abs(q).max(initial=0.0) * s <= ref.IMG_MAX
    hq, rho_q = ref.image(q, k_int, s)
    he, rho_e = ref.image(e, k_int, s)
    rho = rho_q[:, None] + (rho_e.max() if len(rho_e) else 0.0)
    truth = ref.true_sum(q, e, k_int)
    chain = -_rotate_ref.chain_f32(q, e).astype(np.float64)
    c = ref.cmp_int(chain.astype(F32))
    worst = 0.0
    for flush in (False, True):
        A = ref.accumulate(hq, he, k_int, flush_sub=flush).astype(np.float64)
        lower, upper = ref.sum_bounds(A, rho, n, s)
        assert np.all(truth >= lower) and np.all(truth <= upper)
        lower, upper = ref.chain_bounds(A, rho, n, s)
        assert np.all(chain >= lower) and np.all(chain <= upper)
        band = np.maximum(upper - A / s, A / s - lower)
        if band.max() > 0:
            worst = max(worst, float((np.abs(A / s - chain) / np.where(band > 0, band, 1.0)).max()))
        for col in range(min(e.shape[0], 3)):          # positives: the first candidates
            p = c[:, col]
            lo, hi = ref.thresholds(p, rho[:, 0], n, s)
            ok = np.abs(p) < 2 ** 31 - 1000
            gt, lt = (A < lo[:, None]) & ok[:, None], (A > hi[:, None]) & ok[:, None]
            assert np.all(c[gt] > np.broadcast_to(p[:, None], c.shape)[gt])
            assert np.all(c[lt] < np.broadcast_to(p[:, None], c.shape)[lt])
    return worst


@pytest.mark.parametrize("kind", ref.TABLES)
@pytest.mark.parametrize("k", ref.KS)
def test_band_in_numpy_against_float64(k, kind):
    ki = 2 * k
    e = ref.entity_table(kind, 131, ki)
    rs = np.random.RandomState(k)
    # query rows as the device makes them: a table row rotated by a phase per coordinate (components up to sqrt(2) max|e|)
    src, th = e[rs.randint(0, len(e), 33)].astype(np.float64), rs.uniform(-np.pi, np.pi, (33, k))
    q = np.concatenate([src[:, :k] * np.cos(th) - src[:, k:] * np.sin(th), src[:, :k] * np.sin(th) + src[:, k:] * np.cos(th)], 1).astype(F32)
    q[0] = e[5]          # a tie with candidate 5 and near-ties with the rows planted below
    e[6] = e[5]
    e[7] = e[5]
    e[7, 0] = np.nextafter(e[7, 0], F32(np.inf))
    worst = _check_band(q, e, ki)
    assert worst <= 1.0
    if kind == "normal":
        assert worst > 0.05      # (the band is not vacuous: a measured error reaches a fair share of it)


def test_single_coordinate_worst_cases():
    """k = 1, operands at half rounding MIDPOINTS (the largest residuals) and one f32 step to either side of them, across binades from
    the half subnormals of the scaled image up to its largest values, both signs, q and e independently"""
    vals = []
    for ex in (-20, -16, -15, -14, -13, -8, -1, 0, 1, 7, 13):
        for m in (0, 1, 511, 1023):
            mid = (1.0 + (m + 0.5) / 1024.0) * 2.0 ** ex          # halfway between two neighbouring halves of this binade
            for v in (mid, np.nextafter(F32(mid), F32(0)), np.nextafter(F32(mid), F32(np.inf)), (1.0 + m / 1024.0) * 2.0 ** ex):
                vals += [float(v), -float(v)]
    vals = np.array(sorted(set(vals)), np.float64)
    # the table's largest entry pins the scale at 1: the values above ARE the scaled operands
    for top in (16384.0, 3.0):
        s = ref.image_scale(top)
        v = (vals / s).astype(F32)
        re_e, im_e = np.meshgrid(v, v[::7])
        e = np.stack([re_e.ravel(), im_e.ravel()], 1)
        e = np.concatenate([e, [[top, -top]]]).astype(F32)
        q = np.stack([v[::3], v[::3][::-1]], 1).astype(F32)
        assert ref.image_scale(float(np.abs(e).max())) == s
        assert _check_band(q, e, 2) <= 1.0


def test_image_scale():
    from emgraph_amd.evaluation import ranking as RK
    for m in (1e-30, 1e-6, 1e-3, 0.3, 1.0, 1.5, 2.0, 100.0, 8192.0, 8192.5, 16384.0):
        s = RK.rotate_image_scale(m)
        assert s == ref.image_scale(m) and np.log2(s) == int(np.log2(s)) and 1.0 <= s <= 2.0 ** 24
        assert s * m <= RK.ROTATE_ENT_MAX and (s == 2.0 ** 24 or 2 * s * m > RK.ROTATE_ENT_MAX)
        # a query component is at most sqrt(2) (1 + 1e-6) max|e|: its image stays inside the refusal limit, so does every difference
        assert s * m * np.sqrt(2) * (1 + 1e-6) <= ref.IMG_MAX and 2 * ref.IMG_MAX <= 65504
    for m in (0.0, 16384.5, 7e4, float("nan"), float("inf")):
        assert RK.rotate_image_scale(m) == 1.0
    assert RK.ROTATE_ENT_MAX == ref.ENT_MAX


def test_auto_resolves_to_the_fast_mode_only_where_it_applies():
    from emgraph_amd.evaluation import ranking as RK
    assert RK.ROTATE_FAST_AUTO is True      # the measured gate (DESIGN.md 4.5 "Exact-fast ranking")
    fast = RK.resolve_auto_precision(L.ROTATE, 200, 8192, 1 << 20)
    assert fast == 2
    assert RK.resolve_auto_precision(L.ROTATE, 32, 128, 32768) == 2 and RK.resolve_auto_precision(L.ROTATE, 2, 128, 32768) == 2
    assert RK.resolve_auto_precision(L.ROTATE, 200, 127, 1 << 20) == 0            # few test triples
    assert RK.resolve_auto_precision(L.ROTATE, 200, 8192, 32767) == 0             # a small table
    assert RK.resolve_auto_precision(L.ROTATE, 200, 8192, 1 << 20, [1, 2, 3]) == 0   # a candidate list
    for link in (L.LINK_TANH, L.LINK_SIGMOID, L.LINK_SOFTPLUS):                   # under a link: the exact kernel
        assert RK.resolve_auto_precision(L.ROTATE, 200, 8192, 1 << 20, None, link) == 0
        assert not RK.link_prefilter_applies(L.ROTATE, link)
    assert RK.resolve_auto_precision(L.TRANSE_P, 200, 8192, 1 << 20) == 0         # the other generic model: unchanged
    assert RK.resolve_auto_precision(L.TRANSE_L1, 200, 8192, 1 << 20) == 2


def test_header_signatures_and_build_list_declare_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "emgraph_hip.h")).read()
    assert re.search(r"^#define EMG_ABI_VERSION 9$", hdr, re.M) and L.ABI_VERSION == 9 and L.ENOSUP == -3
    assert re.search(r"^#define EMG_ENOSUP \(-3\)", hdr, re.M)
    for sym, n_args in NEW_SYMBOLS.items():
        m = re.search(r"\bint(?:64_t)?\s+%s\(([^;]*)\);" % sym, hdr)
        assert m, sym
        assert len(m.group(1).split(",")) == n_args == len(L.SIGNATURES[sym][1]), sym
    with open(os.path.join(ROOT, "emgraph_amd", "csrc", "build.sh")) as f:
        assert re.search(r"\bemg_rank_rotate\b", f.read())
    assert os.path.exists(os.path.join(ROOT, "emgraph_amd", "csrc", "emg_rank_rotate.hip"))
    if os.path.exists(L.LIB_PATH):
        lib = L.load()
        for sym in NEW_SYMBOLS:
            assert hasattr(lib, sym), sym
        assert [lib.emg_eval_rotate_ld(k) for k in (0, 2, 16, 18, 200)] == [0, 16, 16, 32, 208]
        assert lib.emg_eval_prefilter_rotate_segments(0, 5) == 0 and lib.emg_eval_prefilter_rotate_segments(130, 4099) == 64


def test_pinned_refusals_stay():
    """an explicit precision 1 / 2 names RotatE in a NotImplementedError, sharded RotatE ranking stays refused (before any device work)"""
    from emgraph_amd.evaluation.ranking import rank_triples_device
    from emgraph_amd.models import RotatE
    E, R = np.zeros((6, 8), F32), np.zeros((1, 8), F32)
    T = np.array([[0, 0, 1]], np.int32)
    for prec in (1, 2):
        with pytest.raises(NotImplementedError, match="RotatE"):
            rank_triples_device(L.ROTATE, E, R, 8, 1.0, T, precision=prec)
    with pytest.raises(NotImplementedError, match="RotatE"):
        rank_triples_device(L.ROTATE, E, R, 8, 1.0, T, precision="auto", shard=(0, 2))
    for prec in (1, 2, "2"):
        m = RotatE(k=4, embedding_model_params={"eval_precision": prec})
        m.is_fitted = True
        m.ent_to_idx = {"e%d" % i: i for i in range(6)}
        m.rel_to_idx = {"r0": 0}
        m.trained_model_params = [E, R]
        with pytest.raises(NotImplementedError, match="RotatE"):
            m.get_ranks_idx(T)
    assert "'auto'" in RotatE.__doc__ and "explicit 2" in RotatE.__doc__
