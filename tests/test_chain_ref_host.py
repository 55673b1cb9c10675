"""tests/_chain_ref.py, host side (no GPU): the helper the real-valued discovery tests compare with is pinned here, and so is
the discriminating power of the tables it makes — on them the defined chain must differ in bits from other correct-looking
arithmetic often enough that a kernel computing anything else cannot pass by luck."""
import numpy as np
import pytest

from tests import _chain_ref as ref
from tests._dbscan_ref import dbscan_ref
from tests.test_discovery import distances_l2, int_table

F32 = np.float32
K_DISCRIMINATING = (32, 33, 37, 64, 100, 400)     # every k >= 32 of tests/test_discovery_real.py and test_clusters_real.py
N = 257


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


@pytest.mark.parametrize("k", (1, 3, 4, 37, 100, 400))
def test_l2_chain_equals_the_integer_brute_force_on_integer_tables(k):
    rng = np.random.default_rng(300 + k)
    B = int_table(rng, 130, k)
    A = rng.integers(-3, 4, size=(7, k)).astype(F32)
    assert np.array_equal(bits(ref.l2_chain(B, B)), bits(distances_l2(B, B)[0]))
    assert np.array_equal(bits(ref.l2_chain(A, B)), bits(distances_l2(A, B)[0]))


@pytest.mark.parametrize("maker", sorted(ref.MAKERS))
@pytest.mark.parametrize("k", (1, 3, 33, 400))
def test_l2_chain_is_symmetric_with_a_zero_diagonal(maker, k):
    X = ref.MAKERS[maker](N, k)
    D = ref.l2_chain(X, X)
    assert D.dtype == F32 and D.shape == (N, N)
    assert np.array_equal(bits(D), bits(D.T))
    assert (bits(D).diagonal() == 0).all()            # +0, not -0


def test_cosine_chain_is_one_minus_the_dot_chain_in_f32():
    rng = np.random.default_rng(5)
    X = rng.standard_normal((40, 37)).astype(F32)
    X /= np.sqrt((X * X).sum(1, dtype=F32))[:, None]
    D = ref.cosine_chain(X, X)
    assert D.dtype == F32 and np.array_equal(bits(D), bits(D.T))
    for i, j in ((0, 0), (3, 17), (39, 1)):
        acc = F32(0)
        for c in range(37):                           # the product is exact in float64, one rounding per step: fmaf
            acc = F32(np.float64(X[i, c]) * np.float64(X[j, c]) + np.float64(acc))
        assert bits(D[i, j]) == bits(F32(1) - acc)


@pytest.mark.parametrize("maker", sorted(ref.MAKERS))
def test_tables_are_seeded_and_carry_the_planted_rows(maker):
    make = ref.MAKERS[maker]
    for k in (1, 33, 37):
        X = make(N, k)
        assert X.dtype == F32 and X.shape == (N, k) and np.isfinite(X).all()
        assert np.array_equal(bits(X), bits(make(N, k))) and not np.array_equal(bits(X), bits(make(N, k, seed=1)))
        for a, b in ((N - 1, 0), (40, 7), (62, 7), (64, 1)):
            assert np.array_equal(bits(X[a]), bits(X[b]))
        assert np.array_equal(bits(X[5]), bits(np.nextafter(X[3], F32(np.inf)))) and (X[5] != X[3]).all()
        assert np.array_equal(bits(X[9, :k - 1]), bits(X[8, :k - 1])) and X[9, k - 1] != X[8, k - 1]
        D = ref.l2_chain(X, X)
        assert D[N - 1, 0] == 0 and D[5, 3] > 0 and bits(D[9, 8]) == bits(np.abs(X[9, k - 1] - X[8, k - 1]))
    for n in (1, 2, 63, 64, 65):                      # the small tables plant what they have room for
        X = make(n, 5)
        assert X.shape == (n, 5) and (n < 2 or np.array_equal(bits(X[n - 1]), bits(X[0])))


@pytest.mark.parametrize("maker", sorted(ref.MAKERS))
@pytest.mark.parametrize("k", K_DISCRIMINATING)
def test_tables_separate_the_chain_from_other_arithmetic(maker, k):
    """A condition on the INPUTS: more than a quarter of the off-diagonal chain distances differ in bits from the correctly
    rounded float64 distance, and from a two-accumulator (even k / odd k) chain."""
    X = ref.MAKERS[maker](N, k)
    off = ~np.eye(N, dtype=bool)
    D = ref.l2_chain(X, X)
    frac64 = (bits(D) != bits(ref.float64_l2(X, X)))[off].mean()
    even, odd = np.zeros((N, N), F32), np.zeros((N, N), F32)
    for c in range(k):                                # fmaf: the square is exact in float64, one rounding per step
        d = (X[:, None, c] - X[None, :, c]).astype(np.float64)
        acc = even if c % 2 == 0 else odd
        acc[...] = (d * d + acc.astype(np.float64)).astype(F32)
    frac2 = (bits(D) != bits(np.sqrt(even + odd)))[off].mean()
    print("%s k %d: %.3f of the pairs differ from float64, %.3f from two accumulators" % (maker, k, frac64, frac2))
    assert frac64 > 0.25
    assert frac2 > 0.25


def test_brute_keeps_the_contract_at_inf_and_nan():
    inf, nan = np.inf, np.nan
    dist = np.array([[0, inf, inf, nan],
                     [inf, 0, 2, nan],
                     [inf, 2, 0, nan],
                     [nan, nan, nan, nan]], F32)
    count, nn_dist, nn_id, pairs = ref.brute(dist, 0, 2.0)
    assert count.tolist() == [0, 1, 1, 0]
    assert nn_id.tolist() == [1, 2, 1, -1]            # row 0: every other row at +inf, the lowest OTHER id; row 3: none
    assert np.array_equal(bits(nn_dist), bits(np.array([inf, 2, 2, inf], F32)))
    assert pairs.tolist() == [(1 << 32) | 2, (2 << 32) | 1]
    count, _, nn_id, pairs = ref.brute(dist, 0, inf)  # +inf is within an infinite radius, a NaN is not
    assert count.tolist() == [2, 2, 2, 0] and len(pairs) == 6
    count, nn_dist, nn_id, pairs = ref.brute(dist[1:3], 1, 1.0)      # a slice: rows 1 and 2 of the table
    assert count.tolist() == [0, 0] and nn_id.tolist() == [2, 1] and len(pairs) == 0
    count, nn_dist, nn_id, pairs = ref.brute(dist[:1], -1, 0.0)      # foreign: column 0 is another row, at distance 0
    assert count.tolist() == [1] and nn_id.tolist() == [0] and pairs.tolist() == [0]
    count, nn_dist, nn_id, pairs = ref.brute(np.zeros((1, 1), F32), 0, 5.0)
    assert count.tolist() == [0] and nn_id.tolist() == [-1] and np.isposinf(nn_dist).all() and len(pairs) == 0


def test_neighbours_and_core_eps():
    dist = np.array([[0, 3, 1, 1, 0]], F32)
    ids, out = ref.neighbours(dist, np.array([10, 11, 12, 13, 14]), 7)
    assert ids.tolist() == [[10, 14, 12, 13, 11, -1, -1]] and out[0, :5].tolist() == [0, 0, 1, 1, 3] and np.isinf(out[0, 5:]).all()
    X = ref.blobs(65, 33)
    D = ref.l2_chain(X, X)
    for i in (0, 11, 64):
        for m in (2, 3, 5):
            eps = ref.core_eps(D, i, m)
            assert F32(eps) == np.sort(D[i])[m - 1]
            within = ref.within_matrix(D, eps)
            assert within[i].sum() >= m and dbscan_ref(within, m)[1][i]
            below = np.nextafter(F32(eps), F32(-np.inf))
            assert eps == 0 or ref.within_matrix(D, below)[i].sum() < within[i].sum()


def test_the_matrix_of_a_permuted_table_is_the_permuted_matrix():
    """the chain is a function of the pair: what tests/test_clusters_real.py relies on when it permutes the rows"""
    X = ref.blobs(65, 33)
    order = np.random.default_rng(3).permutation(65)
    assert np.array_equal(bits(ref.l2_chain(X[order], X[order])), bits(ref.l2_chain(X, X)[np.ix_(order, order)]))
