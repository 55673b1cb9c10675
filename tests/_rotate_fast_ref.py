"""Host restatement of the RotatE exact-fast mode's arithmetic (csrc/emg_rank_rotate.hip; the proof: DESIGN.md 4.5 "Exact-fast
ranking"): the half image and its residuals, the prefilter's accumulator, the band and the thresholds — numpy only — and the tables
the tests of tests/test_rotate_fast.py and tests/test_rotate_fast_host.py share."""
import math

import numpy as np

F32 = np.float32
U = 2.0 ** -24             # unit roundoff of f32
HALF_U = 2.0 ** -11        # unit roundoff of half
HALF_MIN = 2.0 ** -14      # smallest normal half
FLUSH = math.sqrt(2.0) * HALF_MIN   # a complex difference whose components may have been flushed
TINY = 2.0 ** -60          # per coordinate: the exact chain's squares may underflow
IMG_MAX = 32752.0
ENT_MAX = 16384.0

KS = (1, 3, 4, 33, 64, 100)
ROWS = (1, 33, 130)
ENTS = (1, 127, 129, 4099)
TABLES = ("normal", "small", "mixed", "zero")
N_REL = 5


def g_a(n):
    """relative error of the prefilter's f32 part: the sum of the squares (1 rounding: half a unit on the root), the root (1 ulp <= 2 u),
    n additions of non-negative terms — (4 + n) u with room"""
    return (4.0 + n) * U * 1.01


def g_s(n):
    """relative error of the canonical f32 chain against the real-valued sum: per coordinate the subtractions, the squares, their
    sum (<= 4 u on the square, 2 u on the root), the root (u), n additions — (6 + n) u with room"""
    return (6.0 + n) * U * 1.01


def image_scale(ent_max):
    if not 0.0 < ent_max <= ENT_MAX:
        return 1.0
    return float(min(2.0 ** (math.frexp(ENT_MAX / ent_max)[1] - 1), 2.0 ** 24))


def image(x, k_int, s):
    """(half image [n, k_int] in the [re | im] column order, rho float64 [n]): x * s rounded to nearest-even half, values below
    the smallest normal half written as zero; rho = sum_j |x_j s - image_j| in float64 (no rounding up: a lower bound of the device's)"""
    xs = np.asarray(x, F32)[:, :k_int] * F32(s)
    h = xs.astype(np.float16)
    h[np.abs(h.astype(F32)) < HALF_MIN] = 0
    res = xs.astype(np.float64) - h.astype(np.float64)
    n = k_int // 2
    return h, np.hypot(res[:, :n], res[:, n:]).sum(1)


def interleaved(h, k_int, ld):
    """the device layout of an image: (re_j, im_j) adjacent, ld columns, padding 0"""
    n = k_int // 2
    out = np.zeros((h.shape[0], ld), np.float16)
    out[:, 0:2 * n:2] = h[:, :n]
    out[:, 1:2 * n:2] = h[:, n:k_int]
    return out


def accumulate(hq, he, k_int, flush_sub=False):
    """the prefilter's accumulator [nq, ne] (scaled units): half subtract, the squares and their sum in f32 (the first square is exact,
    the sum is one fused rounding: computed in float64 and rounded once), the root rounded to f32, f32 additions, j ascending.
    ``flush_sub``: subnormal differences flushed to zero, the other behaviour the band allows"""
    n = k_int // 2
    acc = np.zeros((hq.shape[0], he.shape[0]), F32)
    for j in range(n):
        dr = (hq[:, None, j] - he[None, :, j]).astype(np.float16)
        di = (hq[:, None, n + j] - he[None, :, n + j]).astype(np.float16)
        if flush_sub:
            dr = np.where(np.abs(dr.astype(F32)) < HALF_MIN, np.float16(0), dr)
            di = np.where(np.abs(di.astype(F32)) < HALF_MIN, np.float16(0), di)
        m2 = (dr.astype(np.float64) ** 2 + di.astype(np.float64) ** 2).astype(F32)
        acc = (acc + np.sqrt(m2.astype(np.float64)).astype(F32)).astype(F32)
    return acc


def true_sum(q, e, k_int):
    """sum_j |q_j - e_j| in float64 [nq, ne]"""
    n = k_int // 2
    q, e = np.asarray(q, np.float64), np.asarray(e, np.float64)
    out = np.zeros((q.shape[0], e.shape[0]))
    for j in range(n):
        out += np.hypot(q[:, None, j] - e[None, :, j], q[:, None, n + j] - e[None, :, n + j])
    return out


def sum_bounds(A_scaled, rho, n, s):
    """(lower, upper) of the real-valued sum_j |q_j - e_j| given the prefilter's accumulator (scaled units), rho = rho_q + max rho_e
    (scaled units, broadcastable), n complex coordinates and the scale: the band the thresholds assume, float64"""
    A = np.asarray(A_scaled, np.float64)
    lower = ((A / (1.0 + g_a(n)) - n * FLUSH) / (1.0 + HALF_U) - rho) / s
    upper = ((A / (1.0 - g_a(n)) + n * FLUSH) / (1.0 - HALF_U) + rho) / s
    return lower, upper


def chain_bounds(A_scaled, rho, n, s):
    """(lower, upper) of the canonical f32 chain's accumulator (the exact kernel's -score)"""
    lower, upper = sum_bounds(A_scaled, rho, n, s)
    return lower * (1.0 - g_s(n)) - n * TINY, upper * (1.0 + g_s(n)) + n * TINY


def thresholds(pos_int, rho, n, s):
    """(lo, hi) float64, before the outward rounding to f32: accumulator < lo proves int(score 1e5) > pos_int, > hi proves <"""
    m = -np.asarray(pos_int, np.float64)
    X = (m * 1e-5 / ((1.0 + g_s(n)) * (1.0 + U) * (1.0 + 1e-9)) - n * TINY) * s
    lo = ((X - rho) * (1.0 - HALF_U) - n * FLUSH) * (1.0 - g_a(n)) * (1.0 - 1e-9)
    Y = ((m + 1.0) * 1e-5 * (1.0 + 1e-9) / ((1.0 - g_s(n)) * (1.0 - U)) + n * TINY) * s
    hi = ((Y + rho) * (1.0 + HALF_U) + n * FLUSH) * (1.0 + g_a(n)) * (1.0 + 1e-9)
    return np.where(lo > 1e-30, lo, 0.0), hi


def cmp_int(acc32):
    """int(score * 1e5) of the exact kernel: one rounded f32 product of -acc, truncated"""
    with np.errstate(over="ignore", invalid="ignore"):
        p = (-np.asarray(acc32, F32)) * F32(100000.0)
    return np.clip(np.trunc(p.astype(np.float64)), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)


def entity_table(kind, n_ent, k_int, seed=0):
    rs = np.random.RandomState(1000 * seed + 7 * n_ent + k_int)
    if kind == "normal":
        return (rs.randn(n_ent, k_int) * 0.3).astype(F32)
    if kind == "small":
        return (rs.randn(n_ent, k_int) * 1e-3).astype(F32)
    if kind == "mixed":   # entries of 1e-6 beside entries of 100: half subnormals after the image's scale, no relative precision left
        mag = np.where(rs.rand(n_ent, k_int) < 0.5, 1e-6, 100.0) * rs.uniform(0.5, 1.0, (n_ent, k_int))
        return (mag * rs.choice([-1.0, 1.0], (n_ent, k_int))).astype(F32)
    if kind == "zero":
        return np.zeros((n_ent, k_int), F32)
    raise ValueError(kind)


def relation_table(k_int, seed=0):
    rs = np.random.RandomState(77 + seed + k_int)
    R = np.zeros((N_REL, k_int), F32)
    R[:, :k_int // 2] = rs.uniform(-np.pi, np.pi, (N_REL, k_int // 2))
    return R


def triples(n, n_ent, seed=0, s_below=None):
    """n triples; subjects below ``s_below`` (rows a test never plants), objects from s_below on where the table has them"""
    rs = np.random.RandomState(31 + seed + n + n_ent)
    s_hi = min(s_below or n_ent, n_ent)
    o_lo = s_hi if (s_below and n_ent > 2 * s_below) else 0
    return np.stack([rs.randint(0, s_hi, n), rs.randint(0, N_REL, n), rs.randint(o_lo, n_ent, n)], 1).astype(np.int32)
